"""The float32 restatement of the accelerated sparse coding (tests/fista_ref.py) on the CPU: it is the
oracle's ISTA when the momentum is off, the plain iteration for Nit <= 2 (beta_1 = 0), and with the
soft threshold it never ends above ISTA's lasso objective at the same Nit."""
import numpy as np
import pytest

import fista_ref as F
from oracle import oracle as O

# (bb, nb, Nit, variant, K): the soft-prox shapes of tests/test_gpu_ista_accel.py
SOFT_CASES = [(20, 37, 10, "soft", 256), (36, 30, 30, "soft", 256), (8, 70, 30, "soft", 256),
              (8, 40, 12, "soft", 1024), (36, 12, 6, "soft", 100)]


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.mark.parametrize("bb,nb,Nit,variant,K", [(36, 20, 12, "fro4", 256), (8, 33, 20, "spec2", 100),
                                                  (8, 21, 10, "fro4", 7), (36, 5, 8, "matlab", 256)] + SOFT_CASES)
def test_plain_restatement_is_the_oracle(bb, nb, Nit, variant, K):
    """accel off against oracle.ista_batch at 1e-6 per block (measured: 1.4e-7 at most)."""
    D, Yb, obs, alpha, thr, prox = F.case(bb, nb, variant, K, bb * 1000 + nb + K)
    X, PHI = F.ista(Yb, obs, D, alpha, thr, Nit, prox, accel=False)
    Xo, PHIo = O.ista_batch(Yb, obs, D, alpha, thr, Nit, prox)
    ex = max(rel(X[j], Xo[j]) for j in range(nb))
    ep = max(rel(PHI[j], PHIo[j]) for j in range(nb))
    print(f"plain restatement vs oracle ({bb}, {nb}, {Nit}, {variant}, {K}): coefs {ex:.3e}, phi {ep:.3e}")
    assert ex < 1e-6 and ep < 1e-6


@pytest.mark.parametrize("Nit", [1, 2])
@pytest.mark.parametrize("variant", ["fro4", "soft"])
def test_two_iterations_carry_no_momentum(Nit, variant):
    D, Yb, obs, alpha, thr, prox = F.case(8, 19, variant, 100, 11)
    a = F.ista(Yb, obs, D, alpha, thr, Nit, prox, accel=True)
    b = F.ista(Yb, obs, D, alpha, thr, Nit, prox, accel=False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    c = F.ista(Yb, obs, D, alpha, thr, 3, prox, accel=True)
    d = F.ista(Yb, obs, D, alpha, thr, 3, prox, accel=False)
    assert not np.array_equal(c[0], d[0])          # the third iteration is the first to differ


def test_beta_sequence():
    b = F.betas(4)
    t2 = (1 + np.sqrt(5.0)) / 2
    t3 = (1 + np.sqrt(1 + 4 * t2 * t2)) / 2
    assert b.dtype == np.float32 and b[0] == 0
    assert b[1] == np.float32((t2 - 1) / t3)
    assert np.all(np.diff(b) > 0) and b[-1] < 1


@pytest.mark.parametrize("bb,nb,Nit,variant,K", SOFT_CASES)
def test_fista_lasso_objective_not_above_ista(bb, nb, Nit, variant, K):
    """||m .* (y - D x)||^2 + lambda ||x||_1 per block after FISTA <= after ISTA at the same Nit, with
    a 1e-6 relative allowance for rounding where both have converged."""
    D, Yb, obs, alpha, thr, prox = F.case(bb, nb, variant, K, bb * 1000 + nb + K)
    Xa, _ = F.ista(Yb, obs, D, alpha, thr, Nit, prox, accel=True)
    Xp, _ = F.ista(Yb, obs, D, alpha, thr, Nit, prox, accel=False)
    fa, fp = F.lasso_objective(Yb, obs, D, Xa, 0.1), F.lasso_objective(Yb, obs, D, Xp, 0.1)
    print(f"lasso objective ({bb}, {nb}, {Nit}, {K}): mean FISTA {fa.mean():.6g}, ISTA {fp.mean():.6g}, "
          f"largest ratio {np.max(fa / fp):.9f}")
    assert np.all(fa <= fp * (1 + 1e-6))


def test_warm_start_restarts_the_momentum():
    """x0 given: the run starts there with t = 1, so two accelerated halves are not one run."""
    D, Yb, obs, alpha, thr, prox = F.case(8, 9, "soft", 64, 5)
    X1, _ = F.ista(Yb, obs, D, alpha, thr, 6, prox, accel=True)
    Xh, _ = F.ista(Yb, obs, D, alpha, thr, 3, prox, accel=True)
    X2, _ = F.ista(Yb, obs, D, alpha, thr, 3, prox, accel=True, x0=Xh)
    assert not np.array_equal(X1, X2)
    Ph, _ = F.ista(Yb, obs, D, alpha, thr, 3, prox, accel=False)
    P2, _ = F.ista(Yb, obs, D, alpha, thr, 3, prox, accel=False, x0=Ph)
    assert np.array_equal(P2, F.ista(Yb, obs, D, alpha, thr, 6, prox, accel=False)[0])

"""The CPU model of the step-size kernel (tests/alpha_emu.py) against the fp64 SVD, and the proof that
the inputs of tests/test_gpu_alpha.py are hard for the algorithm and easy for the reference.

Pinned figures are float32 ulp distances of the model's alpha to float32(sigma_max)^2 from the fp64 SVD.
"""
import math

import numpy as np
import pytest

import alpha_emu as E

# (n, K, spectrum) -> ulp of one 128-step run.  Every other hard input gives 0.
CAP128_ULP = {(300, 256, "packed_quad"): 16, (600, 512, "packed_quad"): 8}


def test_tridiagonal_top_and_vector_vs_eigh():
    rng = np.random.default_rng(1)
    for k in (1, 2, 7, 128):
        al = rng.standard_normal(k)
        be = np.abs(rng.standard_normal(k))
        T = np.diag(al) + np.diag(be[:k - 1], 1) + np.diag(be[:k - 1], -1)
        lam, V = np.linalg.eigh(T)
        lmax, hi = E.tri_top(al, be, k)
        # eigh's own backward error is of the order k eps ||T||; bisection's is a few eps ||T||
        assert abs(lmax - lam[-1]) <= (k + 4) * 2.3e-16 * np.abs(lam).max()
        assert hi >= lmax
        z = E.tri_vec(al, be, k, hi)
        assert abs(abs(float(z @ V[:, -1])) - 1.0) < 1e-10
        assert np.linalg.norm(T @ z - lmax * z) < 1e-12 * np.abs(lam).max()


@pytest.mark.parametrize("K", [1, 7, 63, 64, 65, 100, 255, 256, 257, 300])
def test_complete_run_is_exact(K):
    """m = min(m_obs, K) <= 128: the run spans the space, so the model and the fp64 SVD agree to the
    float32 bit on random dictionaries and masks, on either side of the m_obs <= K switch."""
    n = 64
    D = E.random_dictionary(n, K, 3)
    for m_obs in (0, 1, 2, 31, 64):
        obs = E.mask_with(n, m_obs, K)
        info = {}
        a = E.alpha_model(D, obs, info=info)
        assert info["m"] == min(m_obs, K) and info["cycles"] <= 1 and info["steps"] <= max(info["m"], 0)
        assert E.ulp32(a, E.alpha_ref(D[obs.astype(bool)])) == 0
    assert E.alpha_model(D, np.zeros(n, np.uint8)) == np.float32(1.0)


@pytest.mark.parametrize("m_obs", [99, 100, 101, 127, 128, 129, 300])
def test_side_switch_and_step_cap(m_obs):
    n, K = (400, 100) if m_obs < 127 else (400, 300)
    D = E.random_dictionary(n, K, 5)
    obs = E.mask_with(n, m_obs, 5)
    info = {}
    a = E.alpha_model(D, obs, info=info)
    assert info["m"] == min(m_obs, K)
    assert E.ulp32(a, E.alpha_ref(D[obs.astype(bool)])) == 0
    assert info["cycles"] == 1          # a Gaussian dictionary passes the residual check at once


@pytest.mark.parametrize("name", E.SPECTRA)
@pytest.mark.parametrize("n,K", E.HARD_SHAPES)
def test_hard_inputs_pinned(n, K, name):
    H = E.hard_matrix(name, n, K)
    obs = np.ones(n, np.uint8)
    s = np.linalg.svd(H.astype(np.float64), compute_uv=False)
    ref = E.alpha_ref(H)
    # easy for the reference: sigma_max sits at least 1e-3 float32 ulp from a rounding boundary, twelve
    # decades above the fp64 SVD's error
    ulp = float(np.spacing(np.float32(s[0])))
    frac = (s[0] / ulp) % 1.0
    assert abs(frac - 0.5) > 1e-3, frac
    # hard for the algorithm: one 128-step run (the kernel before the restart) at its pinned distance
    one = E.alpha_model(H, obs, cycles=1)
    assert E.ulp32(one, ref) == CAP128_ULP.get((n, K, name), 0)
    assert one <= ref                    # a Ritz value is never above lambda_max
    # the complete run and the restarted one are exact
    assert E.ulp32(E.alpha_model(H, obs, cap=None, cycles=1), ref) == 0
    info = {}
    assert E.ulp32(E.alpha_model(H, obs, info=info), ref) == 0
    assert info["steps"] <= E.CYCLES * E.LANCZOS_MAX
    if name == "all_equal":
        assert info["steps"] == 1        # breakdown at the first step
    elif name == "packed_quad":
        assert info["cycles"] == E.CYCLES    # the residual of a packed top outlasts the work bound
    else:
        assert info["cycles"] == 1 and info["resid"] <= E.TOL * info["lmax"]


@pytest.mark.parametrize("n,K", E.HARD_SHAPES)
def test_packed_top_settles_within_the_work_bound(n, K):
    """The restart raises the Ritz value monotonically; the packed top meets the 2-ulp bar from the
    sixth run on, with ten runs of the bound to spare."""
    H = E.hard_matrix("packed_quad", n, K)
    obs = np.ones(n, np.uint8)
    ref = E.alpha_ref(H)
    prev = 0.0
    for c in (1, 2, 4, 6):
        info = {}
        a = E.alpha_model(H, obs, cycles=c, info=info)
        assert info["lmax"] >= prev and a <= ref
        prev = info["lmax"]
    assert E.ulp32(a, ref) == 0


def test_thr_follows_the_oracle():
    from oracle import oracle as O
    H = E.random_dictionary(40, 30, 9)
    for variant in ("spec2", "soft", "matlab"):
        a, t = O.ista_alpha_h(H, 0.1, variant)
        assert E.thr_ref(a, 0.1, variant) == t
    assert math.isclose(E.thr_ref(np.float32(2.0), 0.1, "soft"), 0.025, rel_tol=1e-7)

"""The fp64 restatement of the TV prox (tests/tvprox_ref.py) against what it must satisfy by itself: K^T is
K's adjoint, T is lrs_sstv_f32's regulariser, the duality gap is non-negative and falls to zero, and the
two-element problems have the closed forms the iteration must reach."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sstv_ref  # noqa: E402
import tvprox_ref as R  # noqa: E402

SHAPES = [(1, 1, 1), (1, 5, 7), (3, 1, 6), (3, 6, 1), (2, 2, 2), (4, 9, 11), (5, 8, 12)]
TERMS = {"spatial": (0.7, 0.0, 0.0), "band": (0.0, 0.4, 0.0), "sstv": (0.0, 0.0, 1.3), "all": (0.7, 0.4, 1.3)}


@pytest.mark.parametrize("terms", list(TERMS))
@pytest.mark.parametrize("shape", SHAPES)
def test_adjoint(shape, terms):
    rng = np.random.default_rng(3)
    u = rng.standard_normal(shape)
    w = R.weights(*TERMS[terms])
    Ku = R.K(u, w)
    p = {f: rng.standard_normal(v.shape) for f, v in Ku.items()}
    lhs = sum(float((Ku[f] * p[f]).sum()) for f in w)
    rhs = float((u * R.Kt(p, shape)).sum())
    scale = sum(float(np.abs(Ku[f] * p[f]).sum()) for f in w)
    assert abs(lhs - rhs) <= 1e-12 * max(scale, 1e-300)


@pytest.mark.parametrize("terms", list(TERMS))
@pytest.mark.parametrize("shape", SHAPES)
def test_regulariser_is_the_sstv_term(shape, terms):
    u = np.random.default_rng(5).random(shape)
    w = TERMS[terms]
    want, _ = sstv_ref.closed_form(u, *w, eps=0.0, n_mean=1)
    got = R.regulariser(u, *w)
    assert abs(got - want) <= 1e-12 * max(abs(want), 1e-300)


@pytest.mark.parametrize("terms", list(TERMS))
def test_gap_is_nonnegative_and_falls(terms):
    """(4, 9, 11), seed 11, inputs in [0, 1], tau w = 0.05: the gap at 50, 200 and 800 iterations."""
    z = np.random.default_rng(11).random((4, 9, 11))
    w = tuple(0.05 * (v > 0) for v in TERMS[terms])
    gaps = []
    for n in (50, 200, 800):
        U, p = R.fgp(z, *w, tau=1.0, n_iter=n)
        g = R.gap(U, p, *w, tau=1.0)
        assert g >= 0.0
        gaps.append(g)
    obj = R.objective(U, z, *w, tau=1.0)
    assert gaps[0] > gaps[1] > gaps[2], gaps
    assert gaps[2] < 1e-6 * obj, (gaps, obj)


# two elements: (shape, the term whose difference exists, L)
TWO = [((2, 1, 1), (0.0, 1.0, 0.0), 4.0), ((1, 2, 1), (1.0, 0.0, 0.0), 8.0), ((1, 1, 2), (1.0, 0.0, 0.0), 8.0)]


@pytest.mark.parametrize("shape,unit,L", TWO)
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_two_elements_saturate_at_the_first_step(shape, unit, L, sign):
    """tau w <= |d| / L: p = sign(d) tau w from the first iteration on, u = (z0 + sign(d) tau w, z1 - ...)."""
    z0, d = 0.375, sign * 0.5
    z = np.array([z0, z0 + d]).reshape(shape)
    for tw in (0.5 / L, 0.03125):          # the boundary |d| / L itself, and inside it; both exact in fp32
        w = tuple(0.25 * v for v in unit)
        for n in (1, 2, 7):
            U, _ = R.fgp(z, *w, tau=4.0 * tw, n_iter=n)
            assert np.abs(U.reshape(-1) - np.array([z0 + sign * tw, z0 + d - sign * tw])).max() <= 1e-15


def test_two_elements_reach_the_mean():
    """tau w > |d| / 2 on (2, 1, 1): the solution is the mean; the error e_k = 1/2 (e_{k-1} + beta (e_{k-1} -
    e_{k-2})) contracts by 2^-1/2 per step, so 100 iterations leave far less than 1e-5 |d|."""
    z = np.array([0.25, 0.875]).reshape(2, 1, 1)
    d = 0.625
    U, _ = R.fgp(z, 0.0, 0.5, 0.0, tau=1.0, n_iter=100)
    assert np.abs(U.reshape(-1) - z.mean()).max() <= 1e-5 * d

"""The checker of the DIP loss's TV term (tests/sstv_ref.py) against itself: the closed-form value and gradient
against torch autograd of the same formula, both in fp64 (CPU).

Tolerance 1e-12 relative (to the value; to the largest gradient entry): both sides are fp64 sums of at most 14
terms per element.  eps = 0 runs on grid inputs (multiples of 2^-6 in [0, 4)) with planted ties, where the
gradient must use sign(0) = 0 as torch's abs backward does; the test asserts that a zero difference of every
kind the shape allows is present.
"""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sstv_ref  # noqa: E402

SHAPES = [(1, 1, 1), (1, 5, 7), (3, 1, 6), (3, 6, 1), (2, 2, 2), (4, 9, 11)]
WEIGHTS = {"spatial": (0.05, 0.0, 0.0), "band": (0.0, 0.02, 0.0), "sstv": (0.0, 0.0, 0.03), "all": (0.05, 0.02, 0.03)}


def _input(shape, eps):
    if eps == 0.0:
        return sstv_ref.grid_image(shape).astype(np.float64)
    rng = np.random.default_rng(7 + shape[0] + 31 * shape[1] + 977 * shape[2])
    return rng.random(shape).astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("eps", [0.0, 1e-3])
@pytest.mark.parametrize("wname", list(WEIGHTS))
@pytest.mark.parametrize("shape", SHAPES)
def test_closed_form_equals_autograd(shape, wname, eps):
    o = _input(shape, eps)
    w = WEIGHTS[wname]
    if eps == 0.0:
        zc, possible = sstv_ref.zero_counts(o), sstv_ref.kinds_possible(shape)
        for kind, can in possible.items():
            assert (zc[kind] > 0) == can, (kind, zc)   # sign(0) = 0 is exercised wherever the shape allows
    R, g = sstv_ref.closed_form(o, *w, eps)
    Ra, ga = sstv_ref.autograd(o, *w, eps)
    assert abs(R - Ra) <= 1e-12 * abs(Ra)
    assert float(np.abs(g - ga).max()) <= 1e-12 * float(np.abs(ga).max())


def test_empty_sums():
    """C = 1, H = 1, W = 1: the corresponding sums are empty; a 1 x 1 x 1 image has no term at all."""
    w = WEIGHTS["all"]
    R, g = sstv_ref.closed_form(np.full((1, 1, 1), 2.5), *w, 1e-3)
    assert R == 0.0 and not g.any()
    o = sstv_ref.grid_image((1, 5, 7)).astype(np.float64)
    assert sstv_ref.closed_form(o, 0.0, 0.02, 0.03, 0.0)[0] == 0.0          # one band: no band, no SSTV term
    o = sstv_ref.grid_image((3, 1, 1)).astype(np.float64)
    assert sstv_ref.closed_form(o, 0.05, 0.0, 0.03, 0.0)[0] == 0.0          # one pixel: no spatial, no SSTV term


def test_known_value():
    """A 2 x 2 x 2 image worked by hand: o[c,y,x] = 4c + 2y + x has every first difference constant (dy = 2,
    dx = 1, dc = 4) and every second difference 0."""
    o = np.arange(8, dtype=np.float64).reshape(2, 2, 2)
    R, g = sstv_ref.closed_form(o, 1.0, 1.0, 1.0, 0.0)
    assert R == (4 * 2 + 4 * 1 + 4 * 4 + 0) / 8
    # each element: -1 or +1 from each of the three first differences it ends; the zero second differences add 0
    want = np.array([[[-3, -1], [-1, 1]], [[-1, 1], [1, 3]]], np.float64) / 8
    assert np.array_equal(g, want)

"""The fp64 restatement of the spectral NLM prox (tests/nlmcube_ref.py) against what it must satisfy by itself:
the identities (no search window, a tiny h, a huge sigma, axes of size 1), the symmetry of the patch distance,
equivariance under spatial transposition and flips, the range of the output, and a denoising case."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nlmcube_ref as R  # noqa: E402

SHAPES = [(1, 1, 1), (1, 5, 7), (3, 1, 6), (3, 6, 1), (2, 2, 2), (4, 9, 11), (5, 8, 12)]   # (B, H, W)
PARAMS = [(1, 1), (3, 3), (7, 2), (5, 5), (7, 5)]                                            # (patch_size, patch_distance)


def _cube(shape, seed=1):
    return np.random.default_rng(seed + 7 * shape[0] + 31 * shape[1] + 977 * shape[2]).random(shape)


def test_layout_helpers_invert_each_other():
    z = _cube((4, 9, 11))
    X = R.unfolded(z)
    assert X.shape == (99, 4) and X[3 + 9 * 5, 2] == z[2, 3, 5]       # p = y + H x
    assert np.array_equal(R.image(X, 9, 11), z)


def test_reflection():
    assert R.reflect(np.arange(-7, 9), 1).tolist() == [0] * 16
    assert R.reflect(np.arange(-5, 8), 4).tolist() == [1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1]
    assert R.reflect(np.arange(-4, 6), 2).tolist() == [0, 1, 0, 1, 0, 1, 0, 1, 0, 1]


@pytest.mark.parametrize("shape", SHAPES)
def test_no_window_returns_z(shape):
    z = _cube(shape)
    for ps in (1, 3, 7):
        assert np.array_equal(R.nlm(z, ps, 0, 0.05, 0.0), z)


@pytest.mark.parametrize("shape", [(3, 6, 1), (4, 9, 11), (5, 8, 12)])
def test_tiny_h_returns_z(shape):
    z = _cube(shape)
    for ps, pd in PARAMS:
        assert np.array_equal(R.nlm(z, ps, pd, 1e-4, 0.0), z)


@pytest.mark.parametrize("ps,pd", PARAMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_huge_sigma_is_the_clipped_window_mean(shape, ps, pd):
    z = _cube(shape)
    assert np.abs(R.nlm(z, ps, pd, 0.1, 10.0) - R.window_mean(z, pd)).max() <= 1e-15


def test_window_mean_of_one_column():
    z = _cube((3, 6, 1))
    want = z.mean(axis=(1, 2), keepdims=True)       # rs = 5 covers all six pixels from every pixel
    assert np.abs(R.window_mean(z, 5) - want).max() <= 1e-15


def test_a_single_pixel_returns_itself():
    z = _cube((1, 1, 1))
    for ps, pd in PARAMS:
        assert np.array_equal(R.nlm(z, ps, pd, 0.1, 0.0), z)
    z = _cube((6, 1, 1))
    assert np.array_equal(R.nlm(z, 7, 5, 0.1, 0.0), z)


@pytest.mark.parametrize("ps,pd", PARAMS)
@pytest.mark.parametrize("shape", [(2, 2, 2), (4, 9, 11), (3, 6, 1)])
def test_patch_distance_symmetry(shape, ps, pd):
    """D(p, t) = D(p + t, -t) wherever p + t is inside the image; D(p, 0) = 0."""
    z = _cube(shape)
    B, H, W = shape
    D = R.patch_distances(z, ps, pd)
    assert not D[(0, 0)].any()
    for (ty, tx), Dt in D.items():
        ok = R.inside(H, W, ty, tx)
        ys, xs = np.nonzero(ok)
        back = D[(-ty, -tx)][ys + ty, xs + tx]
        assert np.abs(Dt[ys, xs] - back).max(initial=0.0) <= 1e-13 * max(1.0, Dt.max())


@pytest.mark.parametrize("ps,pd", [(3, 3), (7, 2), (5, 5)])
@pytest.mark.parametrize("shape", [(4, 9, 11), (3, 1, 6), (2, 2, 2)])
def test_equivariance(shape, ps, pd):
    z = _cube(shape)
    u = R.nlm(z, ps, pd, 0.2, 0.02)
    assert np.abs(R.nlm(z.transpose(0, 2, 1), ps, pd, 0.2, 0.02).transpose(0, 2, 1) - u).max() <= 1e-14
    assert np.abs(R.nlm(z[:, ::-1], ps, pd, 0.2, 0.02)[:, ::-1] - u).max() <= 1e-14
    assert np.abs(R.nlm(z[:, :, ::-1], ps, pd, 0.2, 0.02)[:, :, ::-1] - u).max() <= 1e-14


@pytest.mark.parametrize("ps,pd", PARAMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_output_within_the_band_range(shape, ps, pd):
    z = _cube(shape)
    u = R.nlm(z, ps, pd, 0.2, 0.0)
    lo, hi = z.min(axis=(1, 2), keepdims=True), z.max(axis=(1, 2), keepdims=True)
    assert (u >= lo - 1e-15).all() and (u <= hi + 1e-15).all()
    assert np.abs(u - z).max() > 0 or shape == (1, 1, 1)      # ... and h = 0.2 does average something


def test_denoising():
    clean, noisy = R.denoising_case()
    mse = lambda a: float(((a - clean) ** 2).mean())   # noqa: E731
    r33 = mse(R.nlm(noisy, 3, 3, 0.05, 0.05)) / mse(noisy)
    r72 = mse(R.nlm(noisy, 7, 2, 0.05, 0.05)) / mse(noisy)
    print(f"nlm denoising: MSE ratio {r33:.3f} at (3, 3), {r72:.3f} at (7, 2)")
    assert r33 <= 0.3 and r72 < 1.0

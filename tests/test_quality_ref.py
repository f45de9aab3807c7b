"""tests/quality_ref.py, the fp64 restatement the GPU tests of the quality monitor compare against, on closed
forms (no GPU): a restatement that is itself wrong would pass a kernel with the same mistake."""
import numpy as np

import quality_ref as R
from oracle import oracle as O


def _cube(P, B, seed=0):
    rng = np.random.default_rng(seed)
    return rng.random((P, B)).astype(np.float32) + np.float32(0.05)


def test_identical_cubes():
    C = _cube(30, 5)
    r = R.cube_quality(C, C)
    assert np.array_equal(r["psnr_bands"], np.full(5, 100.0))
    assert r["q"][0] == 100.0 and r["q"][2] == 0.0 and r["q"][3] == 30
    assert r["q"][1] <= np.degrees(1e-6)   # acos near 1: sqrt(2 ulp) at the worst


def test_scaled_cube():
    C = _cube(30, 5)
    r = R.cube_quality(2 * C, C)
    assert r["q"][1] <= np.degrees(1e-6)
    assert abs(r["q"][2] - 1.0) < 1e-15
    # mse_b = mean(c^2): the band PSNR in closed form
    want = 10 * np.log10(255 / np.sqrt((C.astype(np.float64) ** 2).mean(0)))
    assert np.allclose(r["psnr_bands"], want, rtol=0, atol=1e-12)


def test_orthogonal_spectra():
    X = np.zeros((6, 4), np.float32)
    C = np.zeros((6, 4), np.float32)
    X[:, 0], X[:, 2] = 1.0, 0.5
    C[:, 1], C[:, 3] = 0.25, 2.0
    r = R.cube_quality(X, C)
    assert abs(r["q"][1] - 90.0) < 1e-12 and r["q"][3] == 6


def test_known_angle_and_zero_norm_pixels():
    X = np.array([[1, 0], [0, 2], [0, 0], [3, 0]], np.float32)
    C = np.array([[1, 1], [1, 0], [1, 1], [0, 0]], np.float32)
    r = R.cube_quality(X, C)
    assert r["q"][3] == 2                                   # the zero spectra of X (row 2) and of C (row 3) are skipped
    assert abs(r["q"][1] - 67.5) < 1e-12                    # mean of 45 and 90 degrees


def test_empty_region():
    X, C = _cube(12, 3, 1), _cube(12, 3, 2)
    r = R.cube_quality(X, C, np.zeros((12, 3), np.uint8))
    assert np.isnan(r["q"][:3]).all() and r["q"][3] == 0
    assert np.isnan(r["psnr_bands"]).all()


def test_region_restricts_every_sum():
    X, C = _cube(12, 3, 1), _cube(12, 3, 2)
    reg = np.zeros((12, 3), np.uint8)
    reg[:5, 0] = 1                      # band 0, rows 0..4 only
    r = R.cube_quality(X, C, reg)
    d = X[:5, 0].astype(np.float64) - C[:5, 0].astype(np.float64)
    assert np.isnan(r["psnr_bands"][1:]).all()
    assert abs(r["psnr_bands"][0] - 10 * np.log10(255 / np.sqrt((d * d).mean()))) < 1e-12
    assert r["q"][0] == r["psnr_bands"][0]                  # the mean is over the bands that have entries
    assert abs(r["q"][2] - np.sqrt((d * d).sum() / (C[:5, 0].astype(np.float64) ** 2).sum())) < 1e-15
    assert r["q"][3] == 5                                   # SAM: the pixels with an entry, over ALL bands
    full = R.cube_quality(X[:5], C[:5])
    assert abs(r["q"][1] - full["q"][1]) < 1e-12


def test_psnr_bands_match_the_oracle():
    H, W, B = 6, 5, 4
    rng = np.random.default_rng(3)
    clean = rng.random((B, H, W)).astype(np.float32)
    C = np.ascontiguousarray(clean.transpose(2, 1, 0).reshape(H * W, B))   # row p = i + H j
    X = C + rng.normal(0, 0.1, C.shape).astype(np.float32)
    X[:, 2] = C[:, 2]                                       # a band with MSE < 1e-10: the reference has no cap there
    r = R.cube_quality(X, C)
    with np.errstate(divide="ignore"):
        want = O.psnr_bands(X, clean)
    keep = r["sse_b"] / r["n_b"] >= 1e-10
    assert list(keep) == [True, True, False, True]
    assert np.allclose(r["psnr_bands"][keep], want[keep], rtol=0, atol=1e-12)
    assert r["psnr_bands"][2] == 100.0


def test_keep_best_rule():
    nan = float("nan")
    assert R.better(1.0, nan, 1) and R.better(1.0, nan, -1)
    assert not R.better(nan, nan, 1) and not R.better(nan, 0.0, -1)
    assert R.better(2.0, 1.0, 1) and not R.better(2.0, 1.0, -1) and R.better(0.5, 1.0, -1)
    assert not R.better(1.0, 1.0, 1) and not R.better(1.0, 1.0, -1)
    snaps = list("abcdef")
    got = R.keep_best([nan, 3.0, 3.0, nan, 5.0, 4.0], 1, snaps)
    assert got[0][2] is None and np.isnan(got[0][0])
    assert [g[2] for g in got[1:]] == ["b", "b", "b", "e", "e"]
    assert got[-1][:2] == (5.0, 4.0)
    got = R.keep_best([2.0, 2.0, 1.0, nan, 1.0], -1, snaps)
    assert [g[2] for g in got] == ["a", "a", "c", "c", "c"] and got[-1][:2] == (1.0, 2.0)

"""The bounds of tests/test_gpu_svt_edges.py, checked without the code under test: on every case of the
matrix (tests/svt_edges.py) float32 LAPACK (oracle.svt) and the numpy restatement of the chain's float32
stage (emu32) meet a quarter of the GPU bar on err_z = ||U - U*||_F / ||Z||_F, and an fp64 eigh of the fp64
Gram meets the singular-value bound.  A case that breaks one of these is changed, not the factor.

Measured over the matrix: LAPACK at most 0.70 of sqrt(B) 2^-24 and emu32 at most 0.49 (both on (3, 2)); the
eigenvalues of the Gram at most 0.31 of (P + 8 B) 2^-53 ||Z||_F^2 (on (5, 1)).

The wide matrix (257 to 512 bands: tests/test_gpu_svt_wide_edges.py) is held to the same three checks.
Measured over it: LAPACK at most 0.41 of sqrt(B) 2^-24 (`tau0` at (968, 321)) and emu32 at most 0.30 (the
dense (1030, 321)); the eigenvalues of the Gram at most 0.002 of the bound (on (3, 300)).
"""
import os
import sys

import numpy as np
import pytest

from oracle import oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import svt_edges as E  # noqa: E402

ALL_CASE_IDS = E.CASE_IDS + E.WIDE_CASE_IDS    # the narrow ids first, as they were
IDS = [f"{P}x{B}-{name}" for P, B, name in ALL_CASE_IDS]


@pytest.mark.parametrize("P,B,name", ALL_CASE_IDS, ids=IDS)
def test_references_meet_a_quarter_of_the_gpu_bar(P, B, name):
    _, Z, tau, Ustar, sref = E.case(P, B, name)
    assert Z.shape == (P, B) and Z.dtype == np.float32 and not Z.flags.writeable
    assert np.linalg.norm(Ustar) > 0 or name == "allbelow"
    bar = np.sqrt(B) * E.EPS32
    assert bar == pytest.approx(E.u_bound(B) / 4)
    e_lapack = E.err_z(O.svt(Z, tau), Z, tau, Ustar)
    e_emu = E.err_z(E.emu32(Z, tau), Z, tau, Ustar)
    print(f"{P}x{B} {name}: err_z LAPACK {e_lapack:.3e} ({e_lapack / bar:.2f} of the bar), emu32 {e_emu:.3e} "
          f"({e_emu / bar:.2f})")
    assert e_lapack <= bar
    assert e_emu <= bar


@pytest.mark.parametrize("P,B,name", ALL_CASE_IDS, ids=IDS)
def test_gram_eigenvalues_meet_the_singular_value_bound(P, B, name):
    _, Z, _, _, sref = E.case(P, B, name)
    Z64 = Z.astype(np.float64)
    lam = np.linalg.eigh(Z64.T @ Z64)[0][::-1]
    s = np.sqrt(np.maximum(lam, 0.0))
    bound = E.s2_bound(P, B, Z)
    r = min(P, B)
    d = np.max(np.abs(s[:r] ** 2 - sref ** 2))
    print(f"{P}x{B} {name}: max |s^2 - s*^2| {d:.3e} ({d / bound:.3f} of the bound)")
    assert d <= bound
    assert np.all(s[r:] <= np.sqrt(bound))


@pytest.mark.parametrize("P,B", E.SPECTRA_SHAPES + E.WIDE_SPECTRA_SHAPES)
def test_thresholds_at_the_ends_of_the_spectrum(P, B):
    _, Z, tau, Ustar, sref = E.case(P, B, "allbelow")
    assert sref[0] < tau and not Ustar.any()          # U* == 0 exactly
    _, Z, tau, Ustar, _ = E.case(P, B, "tau0")
    assert tau == 0.0
    assert np.linalg.norm(Ustar - Z) <= 1e-12 * np.linalg.norm(Z.astype(np.float64))
    _, Z, tau, Ustar, sref = E.case(P, B, "barely")
    assert sref[0] > tau > sref[1]                    # one singular value survives, by 1e-3 relative
    assert (sref[0] - tau) / tau == pytest.approx(1e-3, rel=1e-2)


def test_case_matrix_is_the_list_of_the_ids():
    m = E.case_matrix()
    assert [(Z.shape[0], Z.shape[1], name) for name, Z, _ in m] == E.CASE_IDS
    assert len(m) == 7 * len(E.BANDS) + len(E.EDGE_SHAPES)
    for (name, c), (_, Z, tau) in zip(E.SCALES, [x for x in m if x[0].startswith("scaled") and x[1].shape[1] == 64]):
        Z1, tau1 = E.scaled_unit(197, 64)
        assert tau == c * tau1
        assert np.linalg.norm(Z - c * Z1.astype(np.float64)) <= 2 * E.EPS32 * np.linalg.norm(Z.astype(np.float64))
    for P, B in E.EDGE_SHAPES:
        _, Z, tau, Ustar, _ = E.case(P, B, "dense")
        assert Ustar.any() and 0 < tau < np.linalg.norm(Z.astype(np.float64))


def test_wide_case_matrix_is_the_list_of_the_ids():
    assert len(E.WIDE_CASE_IDS) == 7 * len(E.WIDE_BANDS) + len(E.WIDE_EDGE_SHAPES)
    assert not set(E.WIDE_CASE_IDS) & set(E.CASE_IDS)
    assert all(256 < B <= 512 for _, B, _ in E.WIDE_CASE_IDS)
    for P, B in E.WIDE_SPECTRA_SHAPES:
        assert P == 3 * B + 5
        assert [(Z.shape[0], Z.shape[1], name) for name, Z, _, _, _ in E.cases(P, B)] == \
            [i for i in E.WIDE_CASE_IDS if i[:2] == (P, B)]
    for P, B in E.WIDE_EDGE_SHAPES:
        _, Z, tau, Ustar, _ = E.case(P, B, "dense")
        assert Z.shape == (P, B)
        assert Ustar.any() and 0 < tau < np.linalg.norm(Z.astype(np.float64))

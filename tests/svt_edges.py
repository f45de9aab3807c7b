"""Hard spectra and edge shapes for the SVT prox, with their fp64 reference: a matrix for at most 256 bands
and a wide one for 257 to 512.

The chain (csrc/svt.hip's header) computes U = Z (I - E) with E = V diag(min(tau / s, 1)) V^T from an fp64
eigendecomposition of the Gram and rounds E to float32 before the product.  Where the result is small beside
Z (the largest singular value just above tau) U = Z - Z E cancels, so the design is accurate relative to
||Z||, not to ||U||: err_z() is that measure.  ref64() is the exact operation in fp64, emu32() a numpy
restatement of the design's float32 stage (no port of any kernel): the bounds of tests/test_svt_edges_ref.py
are checked on it and on float32 LAPACK (oracle.svt), without the code under test.

The case matrix: cases(P, B) for the shapes of SPECTRA_SHAPES (seven spectra each) and of EDGE_SHAPES (one
dense Gaussian each), built once per shape with their references, arrays read-only.  The wide matrix
(WIDE_SPECTRA_SHAPES, WIDE_EDGE_SHAPES, WIDE_CASE_IDS: the chains of csrc/svt_wide.h, svt_wide_eig.h and
svt_wide_mw.h) is built by the same functions with the same spectra and bounds, whose derivations do not
depend on the band count.  Needs numpy alone.
"""
import functools

import numpy as np

TAU = float(np.float32(1 / 0.9))
EPS32 = 2.0 ** -24
EPS64 = 2.0 ** -53

# one band count per shape class of csrc/svt_ws.h and both sides of its boundaries: 7, 64, 198 (triangle in
# LDS), 199 (odd; triangle in the workspace, <13, 50> apply), 208 (<16, 64> apply with the <13, 4> Gram),
# 224 (<16, 8> Gram, nb = 7), 256 (nb = 8)
BANDS = (7, 64, 198, 199, 208, 224, 256)
SPECTRA_SHAPES = tuple((3 * B + 5, B) for B in BANDS)
EDGE_SHAPES = (
    (1, 1), (5, 1), (3, 2), (17, 3),                # tiny and odd B (Bp = B + 1 pads a zero row and column)
    (1, 7), (15, 45), (40, 64), (100, 224),         # P < B: a Gram that is rank-deficient by construction
    (63, 16), (64, 16), (65, 16), (257, 33),        # the apply's 64-row edge; empty Gram slabs (P < 256, 257)
)
SCALES = (("scaled1e-4", 1e-4), ("scaled1e3", 1e3))

# 256 < B <= 512.  k_gram_wide works on panels of 64 columns (4 tiles of 16, nt = ceil(B / 16) tiles kept),
# k_svt_apply_f<2, 8, 0> on panels of 128 columns in ceil(B / 8) pairs of k-steps; Bp is B rounded up to even.
#   257  the first wide count, odd (Bp = 258): the fifth Gram panel and the third apply panel hold one
#        column, nt = 17, B mod 8 = 1
#   258  the same Bp without the pad
#   320  five Gram panels exactly, B mod 8 = 0, two and a half apply panels
#   321  one column past 320
#   385  one column past three apply panels and six Gram panels, odd
#   448  the Specim FX10 count: seven Gram panels, three and a half apply panels
#   511  odd with Bp at the cap: the pad is row and column 511
#   512  the cap
WIDE_BANDS = (257, 258, 320, 321, 385, 448, 511, 512)
WIDE_SPECTRA_SHAPES = tuple((3 * B + 5, B) for B in WIDE_BANDS)
WIDE_EDGE_SHAPES = (
    (1, 257), (3, 300),                             # one slab of 4 staged rows; rank 1 and rank 3
    (127, 258), (128, 258), (129, 258),             # the apply's 128-row workgroup edge; P < B: rank-deficient Gram
    (100, 512), (200, 511),                         # P < B at the cap
    (1024, 257), (1025, 257),                       # 32 rows per slab (one LDS chunk exactly); 36 (a second chunk of 4)
    (1030, 321),                                    # a last slab of 22 rows, staged as 24
)


def u_bound(B):
    """The bar on err_z for the GPU chain: rounding E to float32 and forming I - E perturbs F by at most
    2 * 2^-24 * sqrt(B) in Frobenius norm (||E||_F <= sqrt(B)), the float32 accumulation over B terms adds
    about sqrt(B) * 2^-24: 3 units, taken as 4.  The CPU references are held to a quarter of it."""
    return 4.0 * np.sqrt(B) * EPS32


def s2_bound(P, B, Z):
    """The bar on max_k |s_k^2 - s*_k^2|: P * 2^-53 * ||Z||_F^2 is the worst-case forward error of the fp64
    Gram sum and 8 B * 2^-53 * ||G|| the eigensolver's backward error."""
    return (P + 8 * B) * EPS64 * np.linalg.norm(Z.astype(np.float64)) ** 2


def ref64(Z, tau):
    """U* = Us (S - tau)_+ Vh of the fp64 SVD, and the fp64 singular values."""
    Us, S, Vh = np.linalg.svd(np.asarray(Z, np.float64), full_matrices=False)
    return (Us * np.maximum(S - tau, 0.0)) @ Vh, S


def emu32(Z, tau):
    """The chain's float32 stage: eigh of the fp64 Gram, e_k = tau / s_k where s_k > tau else 1,
    E = V diag(e) V^T rounded to float32, F = I - E and Z F in float32."""
    Z = np.asarray(Z, np.float32)
    Z64 = Z.astype(np.float64)
    lam, V = np.linalg.eigh(Z64.T @ Z64)
    s = np.sqrt(np.maximum(lam, 0.0))
    e = np.ones_like(s)
    np.divide(tau, s, out=e, where=s > tau)
    E = ((V * e) @ V.T).astype(np.float32)
    F = np.eye(Z.shape[1], dtype=np.float32) - E
    return Z @ F


def err_z(U, Z, tau, ref=None):
    """||U - U*||_F / ||Z||_F in fp64 (ref: U* where the caller has it already)."""
    Z64 = np.asarray(Z, np.float64)
    Ustar = ref64(Z64, tau)[0] if ref is None else ref
    return float(np.linalg.norm(np.asarray(U, np.float64) - Ustar) / np.linalg.norm(Z64))


def spectrum_case(P, B, s, seed):
    """Z = Q1 diag(s) Q2^T rounded to float32, Q1 and Q2 from the QR of seeded Gaussians; min(P, B)
    singular values."""
    s = np.asarray(s, np.float64)
    r = min(P, B)
    assert s.shape == (r,)
    rng = np.random.default_rng(seed)
    Q1, _ = np.linalg.qr(rng.standard_normal((P, r)))
    Q2, _ = np.linalg.qr(rng.standard_normal((B, r)))
    return ((Q1 * s) @ Q2.T).astype(np.float32)


def spectra(B):
    """The (name, singular values, tau) of the hard spectra at B bands."""
    nc = min(20, B // 2)
    out = [
        ("graded", np.geomspace(10.0, 1e-5, B), TAU),
        ("cluster", np.concatenate([5.0 * (1.0 + 1e-7 * np.arange(nc)), np.geomspace(4.0, 0.2, B - nc)]), TAU),
        ("barely", np.concatenate([[TAU * (1.0 + 1e-3)], 0.5 * TAU * np.linspace(1.0, 0.1, B - 1)]), TAU),
        ("allbelow", np.linspace(1.0, 0.1, B), TAU),
        ("tau0", np.geomspace(3.0, 0.01, B), 0.0),
    ]
    out += [(name, c * np.geomspace(8.0, 0.05, B), c * TAU) for name, c in SCALES]
    return out


def scaled_unit(P, B):
    """The `scaled` spectrum at c = 1: the run whose path and sweep count the scaled cases must repeat."""
    return spectrum_case(P, B, np.geomspace(8.0, 0.05, B), _seed("scaled", B)), TAU


def _seed(name, B):
    # the scaled cases share a seed, so that they are one matrix at three scales (up to float32 rounding)
    names = ("graded", "cluster", "barely", "allbelow", "tau0", "scaled")
    return 1000 * names.index("scaled" if name.startswith("scaled") else name) + B


def edge_case(P, B):
    """Dense Gaussian Z of scale 2, tau = TAU; at B = 1, tau = ||Z|| / 2 so that U != 0."""
    Z = (2.0 * np.random.default_rng(100 * P + B).standard_normal((P, B))).astype(np.float32)
    tau = TAU if B > 1 else 0.5 * float(np.linalg.norm(Z.astype(np.float64)))
    return Z, tau


@functools.lru_cache(maxsize=None)
def cases(P, B):
    """The cases of a shape as a tuple of (name, Z, tau, U*, s*), built once, the arrays read-only."""
    if (P, B) in SPECTRA_SHAPES + WIDE_SPECTRA_SHAPES:
        todo = [(name, spectrum_case(P, B, s, _seed(name, B)), tau) for name, s, tau in spectra(B)]
    else:
        assert (P, B) in EDGE_SHAPES + WIDE_EDGE_SHAPES, (P, B)
        todo = [("dense",) + edge_case(P, B)]
    out = []
    for name, Z, tau in todo:
        Ustar, sref = ref64(Z, tau)
        for a in (Z, Ustar, sref):
            a.setflags(write=False)
        out.append((name, Z, tau, Ustar, sref))
    return tuple(out)


def case(P, B, name):
    return next(c for c in cases(P, B) if c[0] == name)


def case_matrix():
    """Every case as (name, Z, tau): the spectra at SPECTRA_SHAPES, then the edge shapes."""
    return [c[:3] for P, B in SPECTRA_SHAPES + EDGE_SHAPES for c in cases(P, B)]


# ids of the matrix for pytest.mark.parametrize, without building anything
CASE_IDS = ([(P, B, name) for P, B in SPECTRA_SHAPES for name, _, _ in spectra(B)]
            + [(P, B, "dense") for P, B in EDGE_SHAPES])
WIDE_CASE_IDS = ([(P, B, name) for P, B in WIDE_SPECTRA_SHAPES for name, _, _ in spectra(B)]
                 + [(P, B, "dense") for P, B in WIDE_EDGE_SHAPES])

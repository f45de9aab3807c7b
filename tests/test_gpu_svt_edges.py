"""The SVT prox of at most 256 bands on a real MI355X against an fp64 SVD, on hard spectra and edge shapes
(tests/svt_edges.py has the cases and the reference; tests/test_svt_edges_ref.py holds float32 LAPACK and a
numpy restatement of the design to a quarter of the bars below).  Every case runs on the three chains of
lrs_svt_f32 at these band counts: the one-workgroup tridiagonal chain, the same over many workgroups, and
the Jacobi chain, each on a fresh workspace, L2 = None, c2 = 1.

The bars:
  U    err_z = ||U - U*||_F / ||Z||_F <= 4 sqrt(B) 2^-24.  Rounding E to float32 and forming I - E perturbs
       F by at most 2 * 2^-24 sqrt(B) in Frobenius norm (||E||_F <= sqrt(B)) and the float32 accumulation
       over B terms adds about sqrt(B) 2^-24: 3 units, taken as 4.  U = Z (I - E) cancels where U is small
       beside Z, so the chain is accurate relative to ||Z||, not ||U||: on `barely` (the largest singular
       value 1e-3 above tau) float32 LAPACK itself misses 1e-5 relative to ||U|| by 3 to 8 times.
  s    max_k |s_k^2 - s*_k^2| <= (P + 8 B) 2^-53 ||Z||_F^2: P 2^-53 ||Z||_F^2 is the worst-case forward error
       of the fp64 Gram sum, 8 B 2^-53 ||G|| the eigensolver's backward error.  s is non-negative and
       descending, and s[min(P, B):] <= sqrt of that bound.  rel(s, s*) < 1e-9 on `cluster` and `scaled`
       only: d sigma = d lambda / (2 sigma) is not bounded that way on `graded` or a rank-deficient Gram.
  path state word 4 is 1 or 2 on the tridiagonal chains (which of the two is the certificate's decision) and
       3 on the Jacobi chain, which converges in fewer than kMaxSweeps = 40 sweeps.
`allbelow` (U* = 0) leaves rounding noise where LAPACK gives exact zeros: ||U||_F within the U bar.  `tau0`
holds the U bar against Z itself.

Measured (MI355X), the worst value over the matrix per chain and its ratio to the bar:
  tri       err_z 4.1e-8 on (3, 2), 0.12 of the bar (the largest value: 2.4e-7 on (100, 224), 0.07);
            |s^2 - s*^2| 3.6e-15 on (5, 1), 0.31 of the bound
  tri-mw    U, s and the path equal to tri bit for bit on every case
  jacobi    err_z as tri; |s^2 - s*^2| 1.1e-14 on `allbelow` at (26, 7), 0.45 of the bound
Path 2 (the tridiagonal chains' Jacobi fallback): the four rank-deficient shapes (1, 7), (15, 45), (40, 64),
(100, 224), in 6, 13, 14 and 18 sweeps; every other case certified (path 1).  Jacobi sweeps above 20: `graded`
at B = 198, 199, 208, 224, 256 (25, 24, 24, 26, 25).  tau0 gave U == Z bit for bit on every chain and shape.

Two findings (SVT), both of the threshold Jacobi solve, whose rotation rule is
|a_pq| > 1e-7 sqrt(|a_pp a_qq|):
  * on `cluster` (singular values spaced 1e-7 relative, as tight as that threshold) its eigenvalues miss the
    fp64 bar: max |s^2 - s*^2| 1.2e-7 to 3.3e-6, bars all below 1e-9.  At exit ||Off(A)||_F <= 1e-7 tr G, so
    by Weyl the solve promises 1e-7 ||Z||_F^2 and no more; an fp64 numpy restatement of the rule gives the same
    2.6e-6 at (197, 64).  U meets its bar there (0.05).  Tightening the rule would change the bits of every
    Jacobi result, so `cluster` on a Jacobi solve (path 2 or 3) is taken out of the fp64 s bar and of
    rel(s, s*) < 1e-9 and held to the rule's own bound, 1e-7 ||Z||_F^2 (measured: at most 0.04 of it).
  * scaled by 1e-4 or 1e3, float32(c Z) is another matrix by 6e-8 per entry and the Jacobi sweep count moves
    by one at two shapes (13, 12 against 12 at (197, 64); 14, 14 against 13 at (599, 198); equal elsewhere),
    as it does in the numpy restatement.  The path is equal and asserted; the sweep count is asserted where
    the scaling is exact (test_svt_scale_power_of_two: 2^-13 and 2^10, U and s bit for bit as well).
"""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import svt_edges as E  # noqa: E402

pytestmark = pytest.mark.gpu

C2 = np.float32(1 / 0.9)
JACOBI_TOL = 1e-7    # csrc/svt_jacobi.h: a pair rotates while |a_pq| > tol sqrt(|a_pp a_qq|)
CHAINS = {"tri": dict(method="tri"), "tri-mw": dict(method="tri", multi_wg=True), "jacobi": dict(method="jacobi")}
IDS = [f"{P}x{B}-{name}" for P, B, name in E.CASE_IDS]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lrspnp import ops as _ops
    return _ops


def d(a):
    return torch.from_numpy(np.array(a)).cuda()   # a copy: the shared cases are read-only


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def bits(U, s, st):
    return U.view(np.uint32), s.view(np.uint64), (st[4], st[3] if st[4] != 1 else 0)


def same_bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def run(ops, Z, tau, chain, ws=None, L2=None, warm=False, split=False, X=None, U=None):
    """One call on `chain`: U, s and the state words (host).  X / U: device tensors to use instead of fresh ones."""
    P, B = Z.shape
    ws = ops.svt_workspace(P, B, "cuda") if ws is None else ws
    X = d(Z) if X is None else X
    Ld, c2 = (None, 1.0) if L2 is None else (d(L2), C2)
    s = torch.empty(B, dtype=torch.float64, device="cuda")
    kw = CHAINS[chain]
    if split:
        U = torch.empty_like(X)
        ops.svt_gram(X, Ld, c2, ws, warm=warm, method=kw["method"])
        ops.svt_finish(X, Ld, c2, tau, ws, U, s_out=s, warm=warm, **kw)
    else:
        U = ops.svt(X, Ld, c2, tau, ws, U=U, s_out=s, warm=warm, **kw)
    return U.cpu().numpy(), s.cpu().numpy(), ops.svt_state(ws, P, B)


def check(tag, chain, Z, tau, Ustar, sref, U, s, st, extra_u=0.0, check_s=True, cluster=False):
    """The bars of the module docstring on one result; prints the figures before it asserts.  cluster: the
    eigenvalues of a Jacobi solve (path 2 or 3) are held to its stopping rule's bound (the first finding)."""
    P, B = Z.shape
    r = min(P, B)
    e_u, bar_u = E.err_z(U, Z, tau, Ustar), E.u_bound(B) + extra_u
    bar_s = E.s2_bound(P, B, Z)
    if cluster and st[4] in (2, 3):
        bar_s = JACOBI_TOL * np.linalg.norm(Z.astype(np.float64)) ** 2
    e_s = float(np.max(np.abs(s[:r] ** 2 - sref[:r] ** 2)))
    tail = float(s[r:].max()) if r < B else 0.0
    print(f"svt-edge {chain} {tag}: err_z {e_u:.3e} ({e_u / bar_u:.3f} of the bar), |s^2 - s*^2| {e_s:.3e} "
          f"({e_s / bar_s:.3f} of the bound), s tail {tail:.2e}, path {st[4]}, sweeps {st[3]}")
    assert np.isfinite(U).all() and np.isfinite(s).all()
    assert e_u <= bar_u
    assert np.all(s >= 0.0) and np.all(np.diff(s) <= 0.0)
    if check_s:
        assert e_s <= bar_s
        assert tail <= np.sqrt(bar_s)
    if chain == "jacobi":
        assert st[4] == 3, st[:8]
        assert st[3] < 40, st[:8]     # kMaxSweeps: the threshold Jacobi converged
    else:
        assert st[4] in (1, 2), st[:8]


@pytest.mark.parametrize("P,B,name", E.CASE_IDS, ids=IDS)
def test_svt_case_matrix(ops, P, B, name):
    _, Z, tau, Ustar, sref = E.case(P, B, name)
    out = {}
    for chain in CHAINS:
        U, s, st = run(ops, Z, tau, chain)
        out[chain] = bits(U, s, st)
        check(f"{P}x{B} {name}", chain, Z, tau, Ustar, sref, U, s, st, cluster=(name == "cluster"))
        zn = np.linalg.norm(Z.astype(np.float64))
        if name == "allbelow":
            assert np.linalg.norm(U.astype(np.float64)) <= E.u_bound(B) * zn
        if name == "tau0":
            assert np.linalg.norm(U.astype(np.float64) - Z) <= E.u_bound(B) * zn
            print(f"svt-edge {chain} {P}x{B} tau0: U == Z bit for bit: {np.array_equal(U.view(np.uint32), Z.view(np.uint32))}")
        if (name == "cluster" and st[4] == 1) or name.startswith("scaled"):
            assert rel(s, sref) < 1e-9
        if name.startswith("scaled"):
            # the same spectrum at c = 1 takes the same path (the sweep count: test_svt_scale_power_of_two)
            Z1, tau1 = E.scaled_unit(P, B)
            st1 = run(ops, Z1, tau1, chain)[2]
            print(f"svt-edge {chain} {P}x{B} {name}: at c = 1 path {st1[4]}, sweeps {st1[3]}")
            assert st[4] == st1[4], (st[:8], st1[:8])
    # the many-workgroup tridiagonal chain: U, s and the path bit for bit
    assert same_bits(out["tri"], out["tri-mw"])


@pytest.mark.parametrize("P,B", E.SPECTRA_SHAPES)
def test_svt_scale_power_of_two(ops, P, B):
    """A cube and tau scaled by a power of two take the same path in the same rounds and sweeps and give
    the scaled U and s bit for bit: every product and sum scales exactly, so a difference can come from
    the eigensolver's absolute guards (1e-300, 1e-290, pivmin) alone."""
    Z1, tau1 = E.scaled_unit(P, B)
    for chain in CHAINS:
        U1, s1, st1 = run(ops, Z1, tau1, chain)
        for c in (2.0 ** -13, 2.0 ** 10):     # about 1e-4 and 1e3
            U, s, st = run(ops, (np.float32(c) * Z1), c * tau1, chain)
            print(f"svt-edge {chain} {P}x{B} scaled by {c:g}: path {st[4]}, rounds {st[2]}, sweeps {st[3]} "
                  f"(at c = 1: {st1[4]}, {st1[2]}, {st1[3]})")
            assert st[2:5] == st1[2:5]
            assert np.array_equal(U.view(np.uint32), (np.float32(c) * U1).view(np.uint32))
            assert np.array_equal(s, c * s1)


@pytest.mark.parametrize("chain", list(CHAINS))
@pytest.mark.parametrize("B", [64, 199])
def test_svt_edges_l2_c2(ops, B, chain):
    """Z = X + c2 L2 with c2 = float32(1 / 0.9), an even and an odd B: the reference Z in fp64 from the float32
    inputs, the U bar plus 2^-23 for the one rounding of the kernels' float32 Z.  That rounding moves s^2 by
    2^-23 ||Z||^2, far above the fp64 bound: s is held to ||s - s*||_2 <= ||dZ||_F <= 2^-23 ||Z||_F (Mirsky),
    asserted as 1e-6 relative."""
    P = 3 * B + 5
    X = E.case(P, B, "cluster")[1]
    L2 = (0.01 * np.random.default_rng(B).standard_normal((P, B))).astype(np.float32)
    Z64 = X.astype(np.float64) + float(C2) * L2.astype(np.float64)
    Ustar, sref = E.ref64(Z64, E.TAU)
    U, s, st = run(ops, X, E.TAU, chain, L2=L2)
    check(f"{P}x{B} cluster + c2 L2", chain, Z64, E.TAU, Ustar, sref, U, s, st, extra_u=2.0 ** -23, check_s=False)
    assert rel(s, sref) < 1e-6


@pytest.mark.parametrize("chain", list(CHAINS))
@pytest.mark.parametrize("P,B,name", [(197, 64, "graded"), (602, 199, "graded"), (40, 64, "dense")])
def test_svt_edges_split_call(ops, P, B, name, chain):
    """svt_gram then svt_finish equals svt bit for bit, on a graded spectrum and a rank-deficient Gram."""
    _, Z, tau, _, _ = E.case(P, B, name)
    assert same_bits(bits(*run(ops, Z, tau, chain, split=True)), bits(*run(ops, Z, tau, chain)))


@pytest.mark.parametrize("B", [64, 224])    # the triangle in LDS; in the workspace
def test_svt_edges_workspace_history(ops, B):
    """What a workspace held before a call: a warm Jacobi call on zeros (state word 0 says V is not valid) and
    after an unrelated matrix of the same shape meets the bars; a cold call after a call of the other solver
    equals the same call on a fresh workspace bit for bit."""
    P = 3 * B + 5
    _, Z, tau, Ustar, sref = E.case(P, B, "graded")
    _, Zo, tauo, _, _ = E.case(P, B, "cluster")
    U, s, st = run(ops, Z, tau, "jacobi", warm=True)
    check(f"{P}x{B} graded, warm on zeros", "jacobi", Z, tau, Ustar, sref, U, s, st)
    fresh = {c: bits(*run(ops, Z, tau, c)) for c in ("tri", "jacobi")}
    assert same_bits(bits(U, s, st), fresh["jacobi"])      # not valid: the cold solve
    ws = ops.svt_workspace(P, B, "cuda")
    assert run(ops, Zo, tauo, "jacobi", ws=ws)[2][0] == 1
    U, s, st = run(ops, Z, tau, "jacobi", ws=ws, warm=True)
    check(f"{P}x{B} graded, warm after cluster", "jacobi", Z, tau, Ustar, sref, U, s, st)
    for first, then in (("tri", "jacobi"), ("jacobi", "tri")):
        ws = ops.svt_workspace(P, B, "cuda")
        run(ops, Zo, tauo, first, ws=ws)
        assert same_bits(bits(*run(ops, Z, tau, then, ws=ws)), fresh[then]), (first, then)


@pytest.mark.parametrize("chain", list(CHAINS))
@pytest.mark.parametrize("P,B", [(65, 16), (613, 200)])
def test_svt_edges_misaligned_base(ops, P, B, chain):
    """X and U 4 bytes into a larger buffer, B even: the apply kernel's float2 loads of X[row * B + k] are
    then 4-byte aligned only.  include/lrspnp.h asks no alignment of the SVT calls; the result equals the
    aligned call's bit for bit."""
    Z = (2.0 * np.random.default_rng(P + B).standard_normal((P, B))).astype(np.float32)
    Ustar, sref = E.ref64(Z, E.TAU)
    xb = torch.zeros(P * B + 1, dtype=torch.float32, device="cuda")
    ub = torch.zeros(P * B + 1, dtype=torch.float32, device="cuda")
    X, U = xb[1:].view(P, B), ub[1:].view(P, B)
    X.copy_(d(Z))
    assert X.data_ptr() % 8 == 4 and U.data_ptr() % 8 == 4 and X.is_contiguous()
    Um, s, st = run(ops, Z, E.TAU, chain, X=X, U=U)
    check(f"{P}x{B} dense, base + 4 B", chain, Z, E.TAU, Ustar, sref, Um, s, st)
    assert ub[0].item() == 0.0
    assert same_bits(bits(Um, s, st), bits(*run(ops, Z, E.TAU, chain)))

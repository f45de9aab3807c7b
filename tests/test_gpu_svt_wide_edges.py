"""The SVT prox of 257 to 512 bands on a real MI355X against an fp64 SVD, on hard spectra and edge shapes:
the wide matrix of tests/svt_edges.py (WIDE_CASE_IDS; tests/test_svt_edges_ref.py holds float32 LAPACK and
the numpy restatement of the design to a quarter of the bars below, without the code under test).  Every
case runs on the three chains of lrs_svt_f32 at these band counts, each on a fresh workspace, L2 = None:
  wide-jacobi   the default (state path 3);
  wide-tri      wide_tri=True: the tridiagonal chain (path 4, or 5 after its Jacobi fallback);
  wide-tri-mw   wide_tri=True, wide_mw=True: that chain with the many-workgroup reduction (state word 7 is 1).

The bars are those of tests/test_gpu_svt_edges.py, whose derivations do not depend on the band count:
  U    err_z = ||U - U*||_F / ||Z||_F <= 4 sqrt(B) 2^-24 (svt_edges.u_bound);
  s    max_k |s_k^2 - s*_k^2| <= (P + 8 B) 2^-53 ||Z||_F^2 (svt_edges.s2_bound), s non-negative and descending,
       s[min(P, B):] <= sqrt of that bound; rel(s, s*) < 1e-9 on `scaled*`, and on `cluster` where the
       tridiagonal chain certified (path 4).  `cluster` on a Jacobi solve (path 3 or 5) is held to the
       stopping rule's own bound 1e-7 ||Z||_F^2 (SVT findings: the rule of svt_jacobi.h);
  path 3 on wide-jacobi, 4 or 5 on the tridiagonal chains (the certificate's decision); wherever a Jacobi
       solve ran (3, 5) it took fewer than kMaxSweeps = 40 sweeps.
wide-tri and wide-tri-mw take the same path and are held to each other with the bounds of
test_gpu_svt_wide_mw.test_wide_mw_vs_one_workgroup_chain (no bit equality: the reductions sum in another
order): ||U_mw - U_1wg||_F <= 1e-6 ||U_1wg||_F and |s_mw^2 - s_1wg^2| <= 1e-11 max s^2.  On `allbelow` U* = 0
and both U are rounding noise of 1e-15 ||Z||_F that has no digit in common (measured: ||dU|| about 1.3 ||U||), so
the first is taken relative to ||Z||_F there (dU = Z dE: the bound is one on the float32 rounding of E).

Measured (MI355X) over the matrix, the worst value per chain and its ratio to the bar; records, not pass
conditions:
  wide-jacobi   err_z 3.5e-7 on (200, 511), 0.066 of the bar (the largest ratio: 0.074 on (1030, 321));
                |s^2 - s*^2| 0.129 of the bound on (1030, 321) (6.8e-8); `cluster` 1.8e-6 to 2.9e-6, at most
                0.022 of the rule's 1e-7 ||Z||_F^2 (the fp64 bars there are below 1e-8: the narrow suite's
                first finding holds at these widths).  Path 3 on every case.  Sweeps: `graded` 25, 26, 28,
                26, 27, 29, 28, 27 at B = 257 ... 512 of kMaxSweeps = 40 (25 at B = 256), `cluster` 12 to 13,
                the rank-deficient shapes 12 to 19, `tau0` and `scaled*` 14 to 16, every other case 10 to 11.
  wide-tri      err_z as wide-jacobi; |s^2 - s*^2| 0.064 of the bound on (129, 258), and below 0.001 on every
                certified case (`cluster` 3.6e-14 to 6.4e-14).  Path 4 on all 56 spectra and on (1024, 257),
                (1025, 257), (1030, 321); path 5 on the seven shapes with P < B (the B - P zero eigenvalues are
                a cluster inverse iteration cannot separate) in 12, 12, 18, 18, 18, 18 and 19 sweeps.
                Newton-Schulz steps: 0 on 17 certified cases, 1 on 34, 2 on `graded` at every band count but 258,
                where the one-workgroup reduction took 3 = kWtMaxNs (the many-workgroup one 2).
  wide-tri-mw   the path of wide-tri on every case, word 7 = 1; against wide-tri ||dU|| <= 8.5e-9 ||U||
                (`barely` at B = 511; 0 on most cases, 1.4e-12 ||Z|| at most) and max |d s^2| <= 8.9e-16 max s^2.
tau0 gave U == Z bit for bit on every chain and shape.  The power-of-two scalings repeated path, rounds,
sweeps and Newton-Schulz steps and gave the scaled U and s bit for bit on all three chains at all eight band
counts: no absolute guard of the eigen stages acts.  A workspace filled with 1234.5, and one that another
chain had used, changed no bit of a cold call (nine and twelve comparisons).  A warm Jacobi call on `graded`
after an unrelated matrix took 25 to 29 sweeps (cold: 25 and 27): an unrelated basis is no better a start
than the identity, and no worse.  No id ran longer than 4.6 s (the module: 64 s).
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
CHAINS = {"wide-jacobi": {}, "wide-tri": dict(wide_tri=True), "wide-tri-mw": dict(wide_tri=True, wide_mw=True)}
IDS = [f"{P}x{B}-{name}" for P, B, name in E.WIDE_CASE_IDS]


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
    """U, s, the path, the sweeps where a Jacobi solve ran and the Newton-Schulz steps of a tridiagonal chain."""
    return U.view(np.uint32), s.view(np.uint64), (st[4], st[3] if st[4] in (3, 5) else 0, st[5] if st[4] in (4, 5) else 0)


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
        ops.svt_gram(X, Ld, c2, ws, warm=warm, **kw)
        ops.svt_finish(X, Ld, c2, tau, ws, U, s_out=s, warm=warm, **kw)
    else:
        U = ops.svt(X, Ld, c2, tau, ws, U=U, s_out=s, warm=warm, **kw)
    return U.cpu().numpy(), s.cpu().numpy(), ops.svt_state(ws, P, B)


_fresh = {}


def fresh(ops, P, B, name, chain):
    """The cold call of a case of the matrix on `chain` and a fresh workspace, run once: (U, s, state)."""
    key = (P, B, name, chain)
    if key not in _fresh:
        _, Z, tau, _, _ = E.case(P, B, name)
        _fresh[key] = run(ops, Z, tau, chain)
    return _fresh[key]


def check(tag, chain, Z, tau, Ustar, sref, U, s, st, extra_u=0.0, check_s=True, cluster=False):
    """The bars of the module docstring on one result; prints the figures before it asserts.  cluster: the
    eigenvalues of a Jacobi solve (path 3 or 5) are held to its stopping rule's bound."""
    P, B = Z.shape
    r = min(P, B)
    e_u, bar_u = E.err_z(U, Z, tau, Ustar), E.u_bound(B) + extra_u
    bar_s = E.s2_bound(P, B, Z)
    if cluster and st[4] in (3, 5):
        bar_s = JACOBI_TOL * np.linalg.norm(Z.astype(np.float64)) ** 2
    e_s = float(np.max(np.abs(s[:r] ** 2 - sref[:r] ** 2)))
    tail = float(s[r:].max()) if r < B else 0.0
    print(f"svt-wide-edge {chain} {tag}: err_z {e_u:.3e} ({e_u / bar_u:.3f} of the bar), |s^2 - s*^2| {e_s:.3e} "
          f"({e_s / bar_s:.3f} of the bound), s tail {tail:.2e}, path {st[4]}, sweeps {st[3]}, "
          f"Newton-Schulz steps {st[5]}, word 7 {st[7]}")
    assert np.isfinite(U).all() and np.isfinite(s).all()
    assert e_u <= bar_u
    assert np.all(s >= 0.0) and np.all(np.diff(s) <= 0.0)
    if check_s:
        assert e_s <= bar_s
        assert tail <= np.sqrt(bar_s)
    if chain == "wide-jacobi":
        assert st[4] == 3, st[:8]
    else:
        assert st[4] in (4, 5), st[:8]
        assert st[7] == (1 if chain == "wide-tri-mw" else 0), st[:8]
    if st[4] in (3, 5):
        assert st[3] < 40, st[:8]     # kMaxSweeps: the threshold Jacobi converged


@pytest.mark.parametrize("P,B,name", E.WIDE_CASE_IDS, ids=IDS)
def test_wide_case_matrix(ops, P, B, name):
    _, Z, tau, Ustar, sref = E.case(P, B, name)
    zn = np.linalg.norm(Z.astype(np.float64))
    out = {}
    for chain in CHAINS:
        U, s, st = out[chain] = run(ops, Z, tau, chain)
        check(f"{P}x{B} {name}", chain, Z, tau, Ustar, sref, U, s, st, cluster=(name == "cluster"))
        if name == "allbelow":
            assert np.linalg.norm(U.astype(np.float64)) <= E.u_bound(B) * zn
        if name == "tau0":
            assert np.linalg.norm(U.astype(np.float64) - Z) <= E.u_bound(B) * zn
            print(f"svt-wide-edge {chain} {P}x{B} tau0: U == Z bit for bit: "
                  f"{np.array_equal(U.view(np.uint32), Z.view(np.uint32))}")
        if (name == "cluster" and st[4] == 4) or name.startswith("scaled"):
            assert rel(s, sref) < 1e-9
        if name.startswith("scaled"):
            # the same spectrum at c = 1 takes the same path (the sweep count: test_wide_scale_power_of_two)
            Z1, tau1 = E.scaled_unit(P, B)
            st1 = run(ops, Z1, tau1, chain)[2]
            print(f"svt-wide-edge {chain} {P}x{B} {name}: at c = 1 path {st1[4]}, sweeps {st1[3]}")
            assert st[4] == st1[4], (st[:8], st1[:8])
    # the many-workgroup reduction against the one-workgroup chain (module docstring)
    (U1, s1, st1), (Um, sm, stm) = out["wide-tri"], out["wide-tri-mw"]
    dU = np.linalg.norm(Um.astype(np.float64) - U1)
    e_u = dU / (zn if name == "allbelow" else max(np.linalg.norm(U1.astype(np.float64)), 1e-300))
    e_l = np.max(np.abs(sm ** 2 - s1 ** 2)) / np.max(s1 ** 2)
    print(f"svt-wide-edge wide-tri-mw vs wide-tri {P}x{B} {name}: ||dU|| / ||U|| {e_u:.3e} (/ ||Z|| {dU / zn:.3e}), "
          f"max |d s^2| / max s^2 {e_l:.3e}, paths {stm[4]} {st1[4]}")
    assert stm[4] == st1[4], (stm[:8], st1[:8])
    assert e_u <= 1e-6
    assert e_l <= 1e-11


@pytest.mark.parametrize("P,B", E.WIDE_SPECTRA_SHAPES)
def test_wide_scale_power_of_two(ops, P, B):
    """A cube and tau scaled by a power of two take the same path in the same rounds, sweeps and Newton-Schulz
    steps and give the scaled U and s bit for bit: every product and sum scales exactly, so a difference can
    come from the eigen stages' absolute guards (1e-300, 1e-290, pivmin) alone."""
    Z1, tau1 = E.scaled_unit(P, B)
    for chain in CHAINS:
        U1, s1, st1 = run(ops, Z1, tau1, chain)
        for c in (2.0 ** -13, 2.0 ** 10):     # about 1e-4 and 1e3
            U, s, st = run(ops, (np.float32(c) * Z1), c * tau1, chain)
            print(f"svt-wide-edge {chain} {P}x{B} scaled by {c:g}: path {st[4]}, rounds {st[2]}, sweeps {st[3]}, "
                  f"Newton-Schulz steps {st[5]} (at c = 1: {st1[4]}, {st1[2]}, {st1[3]}, {st1[5]})")
            assert st[2:5] == st1[2:5]
            if chain != "wide-jacobi":
                assert st[5] == st1[5]
            assert np.array_equal(U.view(np.uint32), (np.float32(c) * U1).view(np.uint32))
            assert np.array_equal(s, c * s1)


@pytest.mark.parametrize("chain", list(CHAINS))
@pytest.mark.parametrize("B", [257, 320])
def test_wide_l2_c2(ops, B, chain):
    """Z = X + c2 L2 with c2 = float32(1 / 0.9), an odd and an even B: the reference Z in fp64 from the float32
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
    e_s = rel(s, sref)
    print(f"svt-wide-edge {chain} {P}x{B} cluster + c2 L2: rel s {e_s:.3e}")
    assert e_s < 1e-6


@pytest.mark.parametrize("chain", list(CHAINS))
@pytest.mark.parametrize("P,B,name", [(776, 257, "graded"), (129, 258, "dense")])
def test_wide_split_call(ops, P, B, name, chain):
    """svt_gram then svt_finish with the same flags equals svt bit for bit, on a graded spectrum and a
    rank-deficient Gram."""
    _, Z, tau, _, _ = E.case(P, B, name)
    sp = run(ops, Z, tau, chain, split=True)
    print(f"svt-wide-edge {chain} {P}x{B} {name}, split call: path {sp[2][4]}, sweeps {sp[2][3]}")
    assert same_bits(bits(*sp), bits(*fresh(ops, P, B, name, chain)))


@pytest.mark.parametrize("B", [257, 512])
def test_wide_workspace_history(ops, B):
    """What a workspace held before a warm Jacobi call: on zeros (state word 0 says V is not valid) it is the
    cold call bit for bit; after an unrelated matrix of the same shape, solved by the Jacobi chain (its V
    and products A0 = V^T (G V)) or by the tridiagonal chain (which leaves its eigenvectors for that call),
    it meets the bars in fewer than 40 sweeps."""
    P = 3 * B + 5
    _, Z, tau, Ustar, sref = E.case(P, B, "graded")
    _, Zo, tauo, _, _ = E.case(P, B, "cluster")
    U, s, st = run(ops, Z, tau, "wide-jacobi", warm=True)
    check(f"{P}x{B} graded, warm on zeros", "wide-jacobi", Z, tau, Ustar, sref, U, s, st)
    assert same_bits(bits(U, s, st), bits(*fresh(ops, P, B, "graded", "wide-jacobi")))    # not valid: the cold solve
    for first in ("wide-jacobi", "wide-tri"):
        ws = ops.svt_workspace(P, B, "cuda")
        st0 = run(ops, Zo, tauo, first, ws=ws)[2]
        assert st0[0] == 1, st0[:8]
        U, s, st = run(ops, Z, tau, "wide-jacobi", ws=ws, warm=True)
        check(f"{P}x{B} graded, warm after cluster on {first} (path {st0[4]})", "wide-jacobi", Z, tau, Ustar, sref, U, s,
              st)


def test_wide_workspace_history_after_fallback(ops):
    """The hand-over after the tridiagonal chain's Jacobi fallback (path 5: state word 1 names the V buffer the
    fallback's replay wrote): the repeated-value matrix of test_wide_tri_repeated_singular_values (the
    eigenvalue 4 exactly B - 3 times, which the certificate refuses), then a warm Jacobi call on `graded`."""
    B = 300
    P = 3 * B
    rng = np.random.default_rng(B)
    Xr = np.zeros((P, B), np.float32)
    Xr[:B, :B] = 2.0 * np.eye(B, dtype=np.float32)
    Xr[B:, :3] = (0.5 * rng.standard_normal((P - B, 3))).astype(np.float32)
    name, sv, tau = E.spectra(B)[0]
    assert name == "graded"
    Z = E.spectrum_case(P, B, sv, E._seed(name, B))
    Ustar, sref = E.ref64(Z, tau)
    for first in ("wide-tri", "wide-tri-mw"):
        ws = ops.svt_workspace(P, B, "cuda")
        st0 = run(ops, Xr, E.TAU, first, ws=ws)[2]
        print(f"svt-wide-edge {first} {P}x{B} repeated values: path {st0[4]}, sweeps {st0[3]}, state {st0[:8]}")
        assert st0[4] == 5 and st0[0] == 1, st0[:8]
        U, s, st = run(ops, Z, tau, "wide-jacobi", ws=ws, warm=True)
        check(f"{P}x{B} graded, warm after the fallback of {first}", "wide-jacobi", Z, tau, Ustar, sref, U, s, st)


@pytest.mark.parametrize("then", list(CHAINS))
@pytest.mark.parametrize("B", [257, 512])
def test_wide_cold_call_after_another_chain(ops, B, then):
    """A cold call of a chain after a call of each other chain on the same workspace equals the same call on a
    fresh workspace bit for bit: the tridiagonal chain's F is the head of the rotation log, and the
    many-workgroup reduction's scratch the heads of `partial` and `T` (csrc/svt_ws.h)."""
    P = 3 * B + 5
    _, Z, tau, _, _ = E.case(P, B, "graded")
    _, Zo, tauo, _, _ = E.case(P, B, "cluster")
    want = bits(*fresh(ops, P, B, "graded", then))
    for first in CHAINS:
        if first == then:
            continue
        ws = ops.svt_workspace(P, B, "cuda")
        st0 = run(ops, Zo, tauo, first, ws=ws)[2]
        got = run(ops, Z, tau, then, ws=ws)
        same = same_bits(bits(*got), want)
        print(f"svt-wide-edge {then} {P}x{B} graded after cluster on {first} (path {st0[4]}): path {got[2][4]}, "
              f"sweeps {got[2][3]}, bit-equal to the fresh workspace's: {same}")
        assert same, (first, then)


def dirty_workspace(ops, P, B):
    """A workspace whose every byte past the state block (the first 256) is that of the fp64 value 1234.5."""
    ws = ops.svt_workspace(P, B, "cuda")
    n = (ws.numel() - 256) // 8
    ws[256:256 + 8 * n].view(torch.float64).fill_(1234.5)
    rest = ws.numel() - 256 - 8 * n
    if rest:
        ws[256 + 8 * n:] = ws[256:256 + rest]
    assert not ws[:256].any() and ws[256:264].view(torch.float64).item() == 1234.5
    return ws


@pytest.mark.parametrize("chain", list(CHAINS))
@pytest.mark.parametrize("B", [257, 320, 511])
def test_wide_dirty_workspace(ops, B, chain):
    """A cold call ignores what the workspace holds (include/lrspnp.h): on a workspace filled with 1234.5 past
    the state block it gives the zero-filled workspace's result bit for bit.  B = 257 and 511 have the pad row
    and column; the cold flag words 0, WIDE_TRI and WIDE_TRI | WIDE_MW reset the state block themselves."""
    P = 3 * B + 5
    _, Z, tau, Ustar, sref = E.case(P, B, "graded")
    U, s, st = run(ops, Z, tau, chain, ws=dirty_workspace(ops, P, B))
    want = fresh(ops, P, B, "graded", chain)
    same = same_bits(bits(U, s, st), bits(*want))
    print(f"svt-wide-edge {chain} {P}x{B} graded, dirty workspace: path {st[4]}, sweeps {st[3]} (zero-filled: "
          f"{want[2][4]}, {want[2][3]}), bit-equal: {same}")
    check(f"{P}x{B} graded, dirty workspace", chain, Z, tau, Ustar, sref, U, s, st)
    assert same


@pytest.mark.parametrize("chain", list(CHAINS))
@pytest.mark.parametrize("P,B", [(613, 258), (200, 512)])
def test_wide_misaligned_base(ops, P, B, chain):
    """X and U 4 bytes into a larger buffer, B even: the apply kernel's float2 loads of X[row * B + k] are
    then 4-byte aligned only.  include/lrspnp.h asks no alignment of the SVT calls; the result equals the
    aligned call's bit for bit and the word in front of U is untouched."""
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

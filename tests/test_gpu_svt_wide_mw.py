"""The many-workgroup Householder reduction of the wide tridiagonal chain (256 < B <= 512,
LRS_SVT_WIDE_TRI | LRS_SVT_WIDE_MW / wide_tri=True, wide_mw=True) on a real MI355X: one launch per
column, the launch boundary the only synchronisation between workgroups, then the chain of
svt_wide_eig.h unchanged; through the C ABI and up to the solver.

References: the one-workgroup chain (wide_tri=True alone, on a fresh workspace), numpy's float32 LAPACK
SVD (oracle.svt) and an fp64 numpy SVD.  Tolerances: the project's SVT bound, 1e-5 relative L2 against
LAPACK, and 1e-9 on the singular values against fp64 (the bounds of test_gpu_svt_wide_tri.py).  Against
the one-workgroup chain on the same input: two fp64 eigendecompositions of one G, which differ in U only
through the float32 rounding of E (<= 6e-8 per entry), so 1e-6; and both sets of eigenvalues are
certified against the chain's residual threshold kEigRes ||T|| = 1e-11 ||T||, so
|s_mw^2 - s_1wg^2| <= 1e-11 max(s^2) per value.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

C2 = np.float32(1 / 0.9)
TAU = float(np.float32(1 / 0.9))

# the first wide Bp (258: an odd B, so a zero pad column); ragged against 16, 64 and 256; Bp = 512 with
# the zero pad; the cap
SHAPES = [(600, 257, 8, 0.02), (1031, 300, 8, 0.02), (1500, 511, 5, 0.05), (1200, 512, 8, 0.02)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lrspnp import ops as _ops
    return _ops


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def d(a):
    return torch.from_numpy(np.array(a)).cuda()   # a copy: the shared cases are read-only


def low_rank_case(P, B, rank, noise):
    """The data of test_gpu_svt_wide_tri.low_rank_case."""
    rng = np.random.default_rng(P + B)
    Z = (rng.random((P, rank)) @ rng.random((rank, B)) * 0.3 + noise * rng.standard_normal((P, B)))
    X = Z.astype(np.float32)
    L2 = (0.01 * rng.standard_normal((P, B))).astype(np.float32)
    return rng, X, L2


@functools.lru_cache(maxsize=None)
def case(P, B, rank, noise):
    """Inputs and LAPACK references of a shape, computed once for the tests that share it (read-only)."""
    rng, X, L2 = low_rank_case(P, B, rank, noise)
    Z = X + C2 * L2
    ref = O.svt(Z, 1 / 0.9)
    sref = np.linalg.svd(Z.astype(np.float64), compute_uv=False)
    for a in (X, L2, ref, sref):
        a.setflags(write=False)
    return rng, X, L2, ref, sref


def solve(ops, X, L2, ws, **kw):
    """U, s_out of ops.svt with the flags in kw (numpy)."""
    s = torch.empty(X.shape[1], dtype=torch.float64, device="cuda")
    U = ops.svt(d(X), None if L2 is None else d(L2), C2 if L2 is not None else 1.0, TAU, ws, s_out=s, **kw)
    return U.cpu().numpy(), s.cpu().numpy()


MW = {"wide_tri": True, "wide_mw": True}
_solved = {}


def solved(ops, shape, mw):
    """One cold solve of a shared shape on a fresh workspace with the many-workgroup reduction (mw) or
    the one-workgroup chain, computed once: (U, s, state)."""
    key = (shape, mw)
    if key not in _solved:
        P, B = shape[:2]
        _, X, L2, _, _ = case(*shape)
        ws = ops.svt_workspace(P, B, "cuda")
        U, s = solve(ops, X, L2, ws, **(MW if mw else {"wide_tri": True}))
        _solved[key] = (U, s, ops.svt_state(ws, P, B))
    return _solved[key]


def bits(U, s):
    return U.view(np.uint32), s.view(np.uint64)


@pytest.mark.parametrize("shape", SHAPES)
def test_wide_mw_vs_lapack(ops, shape):
    P, B = shape[:2]
    _, _, _, ref, sref = case(*shape)
    U, s, st = solved(ops, shape, True)
    e_u, e_s = rel(U, ref), rel(s, sref)
    print(f"wide mw ({P}, {B}): rel U {e_u:.3e}, rel s {e_s:.3e}, path {st[4]}, Newton-Schulz steps {st[5]}, "
          f"word 7 {st[7]}")
    assert e_u < 1e-5
    assert e_s < 1e-9
    assert st[4] == 4, st[:8]
    assert st[7] == 1, st[:8]
    assert st[0] == 1 and st[1] == (st[5] & 1), st[:8]


@pytest.mark.parametrize("shape", SHAPES)
def test_wide_mw_vs_one_workgroup_chain(ops, shape):
    """Measured: rel U 0 / 0 / 6.0e-10 / 1.0e-9 and max |d s^2| / max s^2 <= 3.4e-16 over the four shapes;
    bounds 1e-6 and 1e-11 (module docstring)."""
    P, B = shape[:2]
    U, s, st = solved(ops, shape, True)
    U1, s1, st1 = solved(ops, shape, False)
    assert st[7] == 1 and st1[7] == 0 and st1[4] == 4, (st[:8], st1[:8])
    e_u = rel(U, U1)
    e_l = np.max(np.abs(s ** 2 - s1 ** 2)) / np.max(s1 ** 2)
    print(f"wide mw vs the one-workgroup chain ({P}, {B}): rel U {e_u:.3e}, max |d s^2| / max s^2 {e_l:.3e}")
    assert e_u <= 1e-6
    assert e_l <= 1e-11


def test_wide_tri_without_the_bit_is_untouched(ops):
    """wide_tri=True alone: word 7 stays 0 and two runs agree bit for bit."""
    shape = SHAPES[1]
    P, B = shape[:2]
    _, X, L2, _, _ = case(*shape)
    U1, s1, st1 = solved(ops, shape, False)
    ws = ops.svt_workspace(P, B, "cuda")
    U2, s2 = solve(ops, X, L2, ws, wide_tri=True)
    st2 = ops.svt_state(ws, P, B)
    assert st1[4] == 4 and st2[4] == 4 and st1[7] == 0 and st2[7] == 0, (st1[:8], st2[:8])
    for a, b in zip(bits(U1, s1), bits(U2, s2)):
        assert np.array_equal(a, b)


def test_wide_mw_rerun_and_split_call_bit_identical(ops):
    """Fixed-order sums across workgroups: two cold calls on fresh workspaces and the split call agree
    bit for bit."""
    shape = SHAPES[1]
    P, B = shape[:2]
    _, X, L2, _, _ = case(*shape)
    Xd, Ld = d(X), d(L2)
    out = []
    for split in (False, False, True):
        ws = ops.svt_workspace(P, B, "cuda")
        s = torch.empty(B, dtype=torch.float64, device="cuda")
        if split:
            U = torch.empty_like(Xd)
            ops.svt_gram(Xd, Ld, C2, ws, **MW)
            ops.svt_finish(Xd, Ld, C2, TAU, ws, U, s_out=s, **MW)
        else:
            U = ops.svt(Xd, Ld, C2, TAU, ws, s_out=s, **MW)
        st = ops.svt_state(ws, P, B)
        assert st[4] == 4 and st[7] == 1, st[:8]
        out.append(bits(U.cpu().numpy(), s.cpu().numpy()))
    for U, s in out[1:]:
        assert np.array_equal(U, out[0][0]) and np.array_equal(s, out[0][1])


def test_wide_mw_repeated_singular_values(ops):
    """The construction of test_wide_tri_repeated_singular_values: the eigenvalue 4 exactly B - 3 = 297
    times, so long runs of already-reduced columns (beta = 0: every workgroup skips the update on the same
    test); the certificate refuses the inverse-iteration basis (path 5)."""
    B = 300
    rng = np.random.default_rng(B)
    P = 3 * B
    X = np.zeros((P, B), np.float32)
    X[:B, :B] = 2.0 * np.eye(B, dtype=np.float32)
    X[B:, :3] = (0.5 * rng.standard_normal((P - B, 3))).astype(np.float32)
    ws = ops.svt_workspace(P, B, "cuda")
    U, _ = solve(ops, X, None, ws, **MW)
    e = rel(U, O.svt(X, 1 / 0.9))
    st = ops.svt_state(ws, P, B)
    print(f"wide mw repeated singular values: rel U {e:.3e}, path {st[4]}, word 7 {st[7]}")
    assert e < 1e-5
    assert st[4] == 5, st[:8]
    assert st[7] == 1, st[:8]


def test_wide_mw_rank_deficient_gram(ops):
    """P = 200 < B = 300: at least 100 zero eigenvalues (f = 1 there).  Path 4 or 5."""
    P, B = 200, 300
    _, X, L2 = low_rank_case(P, B, 8, 0.02)
    ref = O.svt(X + C2 * L2, 1 / 0.9)
    ws = ops.svt_workspace(P, B, "cuda")
    e_j = rel(solve(ops, X, L2, ws)[0], ref)
    ws = ops.svt_workspace(P, B, "cuda")
    U, _ = solve(ops, X, L2, ws, **MW)
    e_t = rel(U, ref)
    st = ops.svt_state(ws, P, B)
    print(f"wide mw rank-deficient ({P}, {B}): rel U {e_t:.3e} (default wide call {e_j:.3e}), path {st[4]}, "
          f"Newton-Schulz steps {st[5]}")
    assert st[4] in (4, 5) and st[7] == 1, st[:8]
    assert e_t <= max(1e-5, 2 * e_j)


def test_wide_mw_is_ignored_up_to_256_bands(ops):
    P, B = 1200, 256
    _, X, L2 = low_rank_case(P, B, 8, 0.02)
    out = []
    for kw in ({}, MW):
        ws = ops.svt_workspace(P, B, "cuda")
        U, s = solve(ops, X, L2, ws, **kw)
        st = ops.svt_state(ws, P, B)
        assert st[4] == 1 and st[7] == 0, st[:8]
        out.append(bits(U, s))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def test_wide_mw_is_ignored_without_the_wide_tridiagonal_chain(ops):
    """B = 300: the bit without wide_tri, and with method='jacobi', launch the default wide call."""
    from lrspnp._lib import LrsError
    shape = SHAPES[1]
    P, B = shape[:2]
    _, X, L2, _, _ = case(*shape)
    ws = ops.svt_workspace(P, B, "cuda")
    Ud, sd = solve(ops, X, L2, ws)
    assert ops.svt_state(ws, P, B)[4] == 3
    for kw in ({"wide_mw": True}, {"method": "jacobi", "wide_tri": True, "wide_mw": True}):
        ws = ops.svt_workspace(P, B, "cuda")
        U, s = solve(ops, X, L2, ws, **kw)
        st = ops.svt_state(ws, P, B)
        assert st[4] == 3 and st[7] == 0, (kw, st[:8])
        assert np.array_equal(bits(U, s)[0], bits(Ud, sd)[0]), kw
    with pytest.raises(LrsError, match="LRS_E_UNSUPPORTED"):
        ops.svt(d(X), d(L2), C2, TAU, ws, multi_wg=True, **MW)


def test_wide_mw_state_hand_over(ops):
    """A warm many-workgroup call takes no warm start; a warm Jacobi call after it starts from its
    eigenvectors, so it needs no more sweeps than a cold Jacobi solve of the same matrix."""
    shape = SHAPES[1]
    P, B = shape[:2]
    _, X, L2, _, _ = case(*shape)
    ws = ops.svt_workspace(P, B, "cuda")
    solve(ops, X, L2, ws, **MW)
    st = ops.svt_state(ws, P, B)
    assert st[4] == 4 and st[7] == 1, st[:8]
    X2 = (X + 1e-3 * np.random.default_rng(7).standard_normal((P, B))).astype(np.float32)
    ref2 = O.svt(X2 + C2 * L2, 1 / 0.9)
    U2, _ = solve(ops, X2, L2, ws, warm=True, **MW)
    st = ops.svt_state(ws, P, B)
    e_t = rel(U2, ref2)
    assert st[4] == 4 and st[7] == 1, st[:8]
    assert e_t < 1e-5
    solve(ops, X2, L2, ws, warm=True)
    st3 = ops.svt_state(ws, P, B)
    wsc = ops.svt_workspace(P, B, "cuda")
    solve(ops, X2, L2, wsc)
    cold = ops.svt_state(wsc, P, B)
    print(f"wide mw hand-over: warm mw rel U {e_t:.3e}; warm Jacobi after it {st3[3]} sweeps (cold Jacobi {cold[3]})")
    assert st3[4] == 3 and cold[4] == 3
    assert st3[3] <= cold[3], (st3[:5], cold[:5])


def test_solver_wide_mw_vs_oracle(ops):
    """The cube of test_solver_wide_tri_vs_oracle (24 x 24 x 320, bb 8, K 64, Nit 20, spec2) with
    svt_wide_solver='tri-mw': two outer iterations against the oracle stepped beside it, X at 1e-5 and the
    duals at ||d lambda|| <= 1e-5 mu ||X||; the chain certifies at each iteration."""
    from lrspnp import LrsPnP, LrsPnPConfig
    from lrspnp._lib import LrsError
    from lrspnp.data import mask_matrix, synthetic_cube, synthetic_dictionary, unfold
    B = 320
    obs_c, _, mask = synthetic_cube(24, 24, B, seed=3)
    Y, M = unfold(obs_c), mask_matrix(mask, B)
    D = synthetic_dictionary(64, 64, 1)
    cfg = LrsPnPConfig(bb=8, sliding=8, Nit=20, variant="spec2", svt_wide_solver="tri-mw")
    s = LrsPnP(Y, M, D, cfg)
    o = O.LrsPnpOracle(Y, M, D, bb=8, sliding=8, Nit=20, variant="spec2")
    for it in range(2):
        s.step()
        o.step()
        torch.cuda.synchronize()
        e_x = rel(s.X.cpu().numpy(), o.X)
        xn = np.linalg.norm(o.X.astype(np.float64))
        e_1 = np.linalg.norm(s.L1.cpu().numpy().astype(np.float64) - o.L1) / (cfg.mu1 * xn)
        e_2 = np.linalg.norm(s.L2.cpu().numpy().astype(np.float64) - o.L2) / (cfg.mu2 * xn)
        st = ops.svt_state(s.svt_ws, s.P, s.B)
        print(f"wide mw solver it {it + 1}: rel X {e_x:.3e}, dL1/(mu1 |X|) {e_1:.3e}, dL2/(mu2 |X|) {e_2:.3e}, "
              f"path {st[4]}, word 7 {st[7]}")
        assert e_x < 1e-5
        assert e_1 <= 1e-5 and e_2 <= 1e-5
        assert st[4] == 4 and st[7] == 1, st[:8]
    with pytest.raises(LrsError, match="svt_wide_solver"):
        LrsPnP(Y, M, D, LrsPnPConfig(bb=8, sliding=8, Nit=20, variant="spec2", svt_wide_solver="qr"))
    with pytest.raises(LrsError, match="256"):
        LrsPnP(Y, M, D, cfg, comm=object())

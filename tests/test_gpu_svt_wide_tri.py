"""The opt-in tridiagonal eigen chain of wide cubes (256 < B <= 512, LRS_SVT_WIDE_TRI / wide_tri=True) on
a real MI355X: Householder reduction, multisection, inverse iteration and back-transformation at 8
registers per lane, the certificate as fp64 matrix-core GEMMs, its Newton-Schulz steps and the Jacobi
fallback, through the C ABI and up to the solver.

Tolerances: the project's SVT bound, 1e-5 relative L2 against numpy's float32 LAPACK SVD (oracle.svt),
and 1e-9 on the singular values against an fp64 numpy SVD.  Against the default wide call on the same
input: both are fp64 eigendecompositions of the same G and differ only through the float32 rounding of
E (<= 6e-8 per entry), so 1e-6.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

C2 = np.float32(1 / 0.9)
TAU = float(np.float32(1 / 0.9))


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
    """The data of test_gpu_kernels.test_svt_kernel_vs_numpy."""
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


def tri(ops, X, L2, ws, **kw):
    s = torch.empty(X.shape[1], dtype=torch.float64, device="cuda")
    U = ops.svt(d(X), None if L2 is None else d(L2), C2 if L2 is not None else 1.0, TAU, ws, s_out=s, wide_tri=True,
                **kw)
    return U.cpu().numpy(), s.cpu().numpy()


# the first Bp over the limit; an odd B (Bp = B + 1); a ragged P; the cap
@pytest.mark.parametrize("P,B,rank,noise", [(600, 257, 8, 0.02), (1031, 300, 8, 0.02), (1500, 511, 5, 0.05),
                                            (1200, 512, 8, 0.02)])
def test_wide_tri_vs_lapack(ops, P, B, rank, noise):
    _, X, L2, ref, sref = case(P, B, rank, noise)
    ws = ops.svt_workspace(P, B, "cuda")
    U, s = tri(ops, X, L2, ws)
    st = ops.svt_state(ws, P, B)
    e_u, e_s = rel(U, ref), rel(s, sref)
    print(f"wide tri ({P}, {B}): rel U {e_u:.3e}, rel s {e_s:.3e}, path {st[4]}, Newton-Schulz steps {st[5]}")
    assert e_u < 1e-5
    assert e_s < 1e-9
    assert st[4] == 4, st[:8]
    assert st[0] == 1 and st[1] == (st[5] & 1), st[:8]


def test_wide_tri_vs_default_wide_path(ops):
    """6.0e-8 measured at (1031, 300); bound 1e-6 (the float32 rounding of E, module docstring)."""
    P, B = 1031, 300
    _, X, L2, _, _ = case(P, B, 8, 0.02)
    Ut, _ = tri(ops, X, L2, ops.svt_workspace(P, B, "cuda"))
    ws = ops.svt_workspace(P, B, "cuda")
    Uj = ops.svt(d(X), d(L2), C2, TAU, ws).cpu().numpy()
    assert ops.svt_state(ws, P, B)[4] == 3
    e = rel(Ut, Uj)
    print(f"wide tri vs the default wide path ({P}, {B}): rel U {e:.3e}")
    assert e <= 1e-6


def test_wide_tri_repeated_singular_values(ops):
    """The construction of test_svt_wide_repeated_singular_values: the eigenvalue 4 exactly B - 3 = 297
    times.  Inverse iteration's basis is not orthogonal there; the certificate refuses it (path 5)."""
    B = 300
    rng = np.random.default_rng(B)
    P = 3 * B
    X = np.zeros((P, B), np.float32)
    X[:B, :B] = 2.0 * np.eye(B, dtype=np.float32)
    X[B:, :3] = (0.5 * rng.standard_normal((P - B, 3))).astype(np.float32)
    ws = ops.svt_workspace(P, B, "cuda")
    U, _ = tri(ops, X, None, ws)
    e = rel(U, O.svt(X, 1 / 0.9))
    st = ops.svt_state(ws, P, B)
    print(f"wide tri repeated singular values: rel U {e:.3e}, path {st[4]}")
    assert e < 1e-5
    assert st[4] == 5, st[:8]


def test_wide_tri_rank_deficient_gram(ops):
    """P = 200 < B = 300: at least 100 zero eigenvalues (f = 1 there).  Path 4 or 5."""
    P, B = 200, 300
    _, X, L2 = low_rank_case(P, B, 8, 0.02)
    ref = O.svt(X + C2 * L2, 1 / 0.9)
    ws = ops.svt_workspace(P, B, "cuda")
    e_j = rel(ops.svt(d(X), d(L2), C2, TAU, ws).cpu().numpy(), ref)
    ws = ops.svt_workspace(P, B, "cuda")
    U, _ = tri(ops, X, L2, ws)
    e_t = rel(U, ref)
    st = ops.svt_state(ws, P, B)
    print(f"wide tri rank-deficient ({P}, {B}): rel U {e_t:.3e} (default wide call {e_j:.3e}), path {st[4]}, "
          f"Newton-Schulz steps {st[5]}")
    assert st[4] in (4, 5), st[:8]
    assert e_t <= max(1e-5, 2 * e_j)


def test_wide_tri_tight_cluster(ops):
    """Z = Q1 diag(s) Q2^T with 20 singular values spaced 1e-7 relative, above tau, among 280 others
    spread over [0.2, 4] (both sides of tau = 1.11).  Path 4 or 5."""
    P, B = 900, 300
    rng = np.random.default_rng(5)
    Q1, _ = np.linalg.qr(rng.standard_normal((P, B)))
    Q2, _ = np.linalg.qr(rng.standard_normal((B, B)))
    s = np.concatenate([5.0 * (1.0 + 1e-7 * np.arange(20)), np.geomspace(4.0, 0.2, B - 20)])
    X = ((Q1 * s) @ Q2.T).astype(np.float32)
    ws = ops.svt_workspace(P, B, "cuda")
    U, sv = tri(ops, X, None, ws)
    st = ops.svt_state(ws, P, B)
    e_u = rel(U, O.svt(X, 1 / 0.9))
    e_s = rel(sv, np.linalg.svd(X.astype(np.float64), compute_uv=False))
    print(f"wide tri tight cluster: rel U {e_u:.3e}, rel s {e_s:.3e}, path {st[4]}, Newton-Schulz steps {st[5]}")
    assert st[4] in (4, 5), st[:8]
    assert e_u < 1e-5
    assert e_s < 1e-9


def test_wide_tri_rerun_bit_identical(ops):
    """Fixed-order sums everywhere: two cold calls on fresh workspaces and the split call agree bit for bit."""
    P, B = 1031, 300
    _, X, L2, _, _ = case(P, B, 8, 0.02)
    Xd, Ld = d(X), d(L2)
    out = []
    for split in (False, False, True):
        ws = ops.svt_workspace(P, B, "cuda")
        s = torch.empty(B, dtype=torch.float64, device="cuda")
        if split:
            U = torch.empty_like(Xd)
            ops.svt_gram(Xd, Ld, C2, ws, wide_tri=True)
            ops.svt_finish(Xd, Ld, C2, TAU, ws, U, s_out=s, wide_tri=True)
        else:
            U = ops.svt(Xd, Ld, C2, TAU, ws, s_out=s, wide_tri=True)
        assert ops.svt_state(ws, P, B)[4] == 4
        out.append((U.cpu().numpy().view(np.uint32), s.cpu().numpy().view(np.uint64)))
    for U, s in out[1:]:
        assert np.array_equal(U, out[0][0]) and np.array_equal(s, out[0][1])


def test_wide_tri_state_hand_over(ops):
    """A warm tridiagonal call needs no warm start; a warm Jacobi call after it starts from its
    eigenvectors, so it needs no more sweeps than a cold Jacobi solve of the same matrix."""
    P, B = 1031, 300
    rng, X, L2, _, _ = case(P, B, 8, 0.02)
    ws = ops.svt_workspace(P, B, "cuda")
    tri(ops, X, L2, ws)
    assert ops.svt_state(ws, P, B)[4] == 4
    X2 = (X + 1e-3 * np.random.default_rng(7).standard_normal((P, B))).astype(np.float32)
    ref2 = O.svt(X2 + C2 * L2, 1 / 0.9)
    U2, _ = tri(ops, X2, L2, ws, warm=True)
    st = ops.svt_state(ws, P, B)
    e_t = rel(U2, ref2)
    assert st[4] == 4, st[:8]
    assert e_t < 1e-5
    U3 = ops.svt(d(X2), d(L2), C2, TAU, ws, warm=True).cpu().numpy()
    st3 = ops.svt_state(ws, P, B)
    e_j = rel(U3, ref2)
    wsc = ops.svt_workspace(P, B, "cuda")
    ops.svt(d(X2), d(L2), C2, TAU, wsc)
    cold = ops.svt_state(wsc, P, B)
    print(f"wide tri hand-over: warm tri rel U {e_t:.3e}; warm Jacobi after it rel U {e_j:.3e}, sweeps {st3[3]} "
          f"(cold Jacobi {cold[3]})")
    assert st3[4] == 3 and cold[4] == 3
    assert e_j < 1e-5
    assert st3[3] <= cold[3], (st3[:5], cold[:5])


def test_wide_tri_is_ignored_up_to_256_bands(ops):
    P, B = 1200, 256
    _, X, L2 = low_rank_case(P, B, 8, 0.02)
    out = []
    for wt in (False, True):
        ws = ops.svt_workspace(P, B, "cuda")
        s = torch.empty(B, dtype=torch.float64, device="cuda")
        U = ops.svt(d(X), d(L2), C2, TAU, ws, s_out=s, wide_tri=wt)
        assert ops.svt_state(ws, P, B)[4] == 1
        out.append((U.cpu().numpy().view(np.uint32), s.cpu().numpy().view(np.uint64)))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def test_wide_tri_refusals(ops):
    from lrspnp._lib import LrsError
    P = 400
    _, X, L2 = low_rank_case(P, 300, 8, 0.02)
    ws = ops.svt_workspace(P, 300, "cuda")
    with pytest.raises(LrsError, match="LRS_E_UNSUPPORTED"):
        ops.svt(d(X), d(L2), C2, TAU, ws, wide_tri=True, multi_wg=True)
    with pytest.raises(LrsError, match="LRS_E_WORKSPACE"):
        ops.svt(d(X), d(L2), C2, TAU, ws[:-1], wide_tri=True)
    X513 = torch.zeros((P, 513), dtype=torch.float32, device="cuda")
    with pytest.raises(LrsError, match="LRS_E_UNSUPPORTED"):
        ops.svt(X513, None, 1.0, TAU, ws, wide_tri=True)
    with pytest.raises(LrsError, match="LRS_E_UNSUPPORTED"):
        ops.svt_gram(X513, None, 1.0, ws, wide_tri=True)


def test_solver_wide_tri_vs_oracle(ops):
    """The cube of test_solver_wide_cube_vs_oracle (24 x 24 x 320, bb 8, K 64, Nit 20, spec2) with
    svt_wide_solver='tri': two outer iterations against the oracle stepped beside it, X at 1e-5 and the
    duals at ||d lambda|| <= 1e-5 mu ||X||; the tridiagonal chain certifies at each iteration."""
    from lrspnp import LrsPnP, LrsPnPConfig
    from lrspnp._lib import LrsError
    from lrspnp.data import mask_matrix, synthetic_cube, synthetic_dictionary, unfold
    B = 320
    obs_c, _, mask = synthetic_cube(24, 24, B, seed=3)
    Y, M = unfold(obs_c), mask_matrix(mask, B)
    D = synthetic_dictionary(64, 64, 1)
    cfg = LrsPnPConfig(bb=8, sliding=8, Nit=20, variant="spec2", svt_wide_solver="tri")
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
        print(f"wide tri solver it {it + 1}: rel X {e_x:.3e}, dL1/(mu1 |X|) {e_1:.3e}, dL2/(mu2 |X|) {e_2:.3e}, "
              f"path {st[4]}")
        assert e_x < 1e-5
        assert e_1 <= 1e-5 and e_2 <= 1e-5
        assert st[4] == 4, st[:8]
    with pytest.raises(LrsError, match="svt_wide_solver"):
        LrsPnP(Y, M, D, LrsPnPConfig(bb=8, sliding=8, Nit=20, variant="spec2", svt_wide_solver="qr"))
    with pytest.raises(LrsError, match="256"):
        LrsPnP(Y, M, D, cfg, comm=object())

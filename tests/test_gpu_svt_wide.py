"""The wide-band SVT path (256 < B <= 512 spectral bands) on a real MI355X: the tiled fp64 Gram, the
one-workgroup Jacobi chain on the workspace triangle and the tiled apply, through the C ABI and up to
the solver.

Tolerances: the project's SVT bound, 1e-5 relative L2 against numpy's float32 LAPACK SVD (the
reference's call; that SVD and an fp64 Gram SVT differ by 0.9e-7 to 4.2e-7 at these shapes), and
1e-9 on the singular values against an fp64 numpy SVD.
"""
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
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def low_rank_case(P, B, rank, noise):
    """The data of test_gpu_kernels.test_svt_kernel_vs_numpy."""
    rng = np.random.default_rng(P + B)
    Z = (rng.random((P, rank)) @ rng.random((rank, B)) * 0.3 + noise * rng.standard_normal((P, B)))
    X = Z.astype(np.float32)
    L2 = (0.01 * rng.standard_normal((P, B))).astype(np.float32)
    return rng, X, L2


# the first Bp over the limit; odd B (Bp = B + 1); P no multiple of 4, 16 or 64; the cap
@pytest.mark.parametrize("P,B,rank,noise", [(600, 257, 8, 0.02), (1031, 300, 8, 0.02), (2000, 448, 8, 0.02),
                                            (1500, 511, 5, 0.05), (1200, 512, 8, 0.02)])
def test_svt_wide_vs_numpy(ops, P, B, rank, noise):
    rng, X, L2 = low_rank_case(P, B, rank, noise)
    ref = O.svt(X + C2 * L2, 1 / 0.9)
    ws = ops.svt_workspace(P, B, "cuda")
    s = torch.empty(B, dtype=torch.float64, device="cuda")
    U = ops.svt(d(X), d(L2), C2, TAU, ws, s_out=s, warm=False, method="tri").cpu().numpy()
    e_u = rel(U, ref)
    sref = np.linalg.svd((X + C2 * L2).astype(np.float64), compute_uv=False)
    e_s = rel(s.cpu().numpy(), sref)
    st = ops.svt_state(ws, P, B)
    print(f"wide SVT ({P}, {B}): rel U {e_u:.3e}, rel s {e_s:.3e}, path {st[4]}, cold sweeps {st[3]}")
    assert e_u < 1e-5
    assert e_s < 1e-9
    assert st[4] == 3, st[:5]     # the Jacobi chain, although the call asked for 'tri'
    cold_sweeps = st[3]
    # warm start from the previous eigenvectors on a perturbed matrix: LRS_SVT_WARM alone
    X2 = (X + 1e-3 * rng.standard_normal((P, B))).astype(np.float32)
    U2 = ops.svt(d(X2), d(L2), C2, TAU, ws, warm=True, method="tri").cpu().numpy()
    e_w = rel(U2, O.svt(X2 + C2 * L2, 1 / 0.9))
    st2 = ops.svt_state(ws, P, B)
    print(f"wide SVT ({P}, {B}) warm: rel U {e_w:.3e}, sweeps {st2[3]}")
    assert e_w < 1e-5
    assert st2[4] == 3 and st2[3] <= cold_sweeps, (st2[:5], cold_sweeps)
    if P == 600:   # once without the dual term
        U0 = ops.svt(d(X), None, 1.0, TAU, ops.svt_workspace(P, B, "cuda")).cpu().numpy()
        e_0 = rel(U0, O.svt(X, 1 / 0.9))
        print(f"wide SVT ({P}, {B}) L2=None: rel U {e_0:.3e}")
        assert e_0 < 1e-5


def test_svt_wide_rerun_bit_identical(ops):
    """No floating-point atomics anywhere in the chain: two cold calls on fresh workspaces agree bit
    for bit, and so does the split call (svt_gram + svt_finish)."""
    P, B = 1031, 300
    _, X, L2 = low_rank_case(P, B, 8, 0.02)
    Xd, Ld = d(X), d(L2)
    out = []
    for split in (False, False, True):
        ws = ops.svt_workspace(P, B, "cuda")
        s = torch.empty(B, dtype=torch.float64, device="cuda")
        if split:
            U = torch.empty_like(Xd)
            ops.svt_gram(Xd, Ld, C2, ws)
            ops.svt_finish(Xd, Ld, C2, TAU, ws, U, s_out=s)
        else:
            U = ops.svt(Xd, Ld, C2, TAU, ws, s_out=s)
        out.append((U.cpu().numpy().view(np.uint32), s.cpu().numpy().view(np.uint64)))
    for U, s in out[1:]:
        assert np.array_equal(U, out[0][0]) and np.array_equal(s, out[0][1])


def test_svt_wide_repeated_singular_values(ops):
    """The exact=True construction of test_gpu_kernels.test_svt_repeated_singular_values: Z = 2 [I; 0]
    plus a rank-3 term on rows the identity does not touch, so the Gram has the eigenvalue 4 exactly
    B - 3 times.  The Jacobi chain's basis is orthogonal whatever the multiplicities."""
    B = 300
    rng = np.random.default_rng(B)
    P = 3 * B
    X = np.zeros((P, B), np.float32)
    X[:B, :B] = 2.0 * np.eye(B, dtype=np.float32)
    X[B:, :3] = (0.5 * rng.standard_normal((P - B, 3))).astype(np.float32)
    ws = ops.svt_workspace(P, B, "cuda")
    U = ops.svt(d(X), None, 1.0, TAU, ws).cpu().numpy()
    e = rel(U, O.svt(X, 1 / 0.9))
    print(f"wide SVT repeated singular values: rel U {e:.3e}")
    assert e < 1e-5
    assert ops.svt_state(ws, P, B)[4] == 3


def test_svt_wide_refusals(ops):
    from lrspnp._lib import LrsError
    P = 400
    small = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")   # the band check comes before the size check
    for B in (513, 514):
        X = torch.zeros((P, B), dtype=torch.float32, device="cuda")
        with pytest.raises(LrsError, match="LRS_E_UNSUPPORTED"):
            ops.svt(X, None, 1.0, TAU, small)
        with pytest.raises(LrsError, match="LRS_E_UNSUPPORTED"):
            ops.svt_gram(X, None, 1.0, small)
    _, X, L2 = low_rank_case(P, 300, 8, 0.02)
    ws = ops.svt_workspace(P, 300, "cuda")
    with pytest.raises(LrsError, match="LRS_E_UNSUPPORTED"):
        ops.svt(d(X), d(L2), C2, TAU, ws, multi_wg=True)
    with pytest.raises(LrsError, match="LRS_E_WORKSPACE"):
        ops.svt(d(X), d(L2), C2, TAU, ws[:-1])
    # the paths of B <= 256 are where they were
    _, X, L2 = low_rank_case(1200, 256, 8, 0.02)
    ws = ops.svt_workspace(1200, 256, "cuda")
    U = ops.svt(d(X), d(L2), C2, TAU, ws, method="tri").cpu().numpy()
    assert ops.svt_state(ws, 1200, 256)[4] == 1
    assert rel(U, O.svt(X + C2 * L2, 1 / 0.9)) < 1e-5


def test_solver_wide_cube_vs_oracle(ops):
    """Two outer iterations of LrsPnP(lowrank='svt'), default SVT settings, on a 24 x 24 x 320 cube
    (P = 576, bb = 8 non-overlapping, seeded K = 64 dictionary, spec2, Nit 20, ~5 % of the pixels
    missing) against the oracle stepped beside it.  X at 1e-5; the duals at X's scale,
    ||d lambda|| <= 1e-5 mu ||X|| (they are mu (X - Phi) and mu (X - U), differences far
    smaller than X).  The second iteration takes the warm-started solve."""
    from lrspnp import LrsPnP, LrsPnPConfig
    from lrspnp._lib import LrsError
    from lrspnp.data import mask_matrix, synthetic_cube, synthetic_dictionary, unfold
    B = 320
    obs_c, _, mask = synthetic_cube(24, 24, B, seed=3)
    Y, M = unfold(obs_c), mask_matrix(mask, B)
    D = synthetic_dictionary(64, 64, 1)
    cfg = LrsPnPConfig(bb=8, sliding=8, Nit=20, variant="spec2")
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
        print(f"wide solver it {it + 1}: rel X {e_x:.3e}, dL1/(mu1 |X|) {e_1:.3e}, dL2/(mu2 |X|) {e_2:.3e}, "
              f"sweeps {st[3]}")
        assert e_x < 1e-5
        assert e_1 <= 1e-5 and e_2 <= 1e-5
        assert st[4] == 3
    with pytest.raises(LrsError, match="256"):
        LrsPnP(Y, M, D, cfg, comm=object())
    Y6 = np.zeros((576, 600), np.float32)
    Y6[:, :B] = Y
    with pytest.raises(LrsError, match="512"):
        LrsPnP(Y6, np.ones_like(Y6), D, cfg)

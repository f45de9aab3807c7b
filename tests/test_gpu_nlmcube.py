"""GPU: the spectral NLM prox on the cube (csrc/nlmcube.hip: lrs_nlmcube_f32, ops.nlmcube) and lowrank="nlm".

Against tests/nlmcube_ref.py (the fp64 restatement of the operator the header defines): bit-exact identities, the
clipped-window mean under a huge sigma, parity over shapes x parameter sets x (h, sigma), the denoising case,
determinism (reruns, an aligned and a misaligned base), the tile seams of a many-workgroup cube, the workspace,
and the solver.

Tolerances.  TOL_U[(patch_size, patch_distance)]: the absolute error of U for inputs in [0, 1], four
times the largest error measured on the MI355X over SHAPES x H_SIGMA (and BIG where it runs) for that parameter
set, against the fp64 restatement.
"""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nlmcube_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

# (B, H, W): sizes below the pads, odd tails in every axis, a band count that is no chunk multiple, the real 198
SHAPES = [(1, 1, 1), (1, 5, 7), (3, 1, 6), (3, 6, 1), (2, 2, 2), (4, 9, 11), (5, 8, 12), (7, 37, 41), (33, 10, 9),
          (198, 12, 9)]
BIG = (31, 70, 50)
PARAMS = [(1, 1), (3, 3), (7, 2), (5, 5), (7, 5)]   # (patch_size, patch_distance)
H_SIGMA = [(0.05, 0.0), (0.05, 0.05), (0.2, 0.0), (0.2, 0.05)]
C2 = 0.5
TILE = 8                                            # the kernel's spatial tile edge
ULP1 = float(np.spacing(np.float32(1.0)))
# measured maxima (MI355X, SHAPES x H_SIGMA, and BIG at (7, 2) and (5, 5)), DESIGN §13: all at h = 0.2 (at h = 0.05
# the weights of a random cube underflow and U = Z to 1e-8 or exactly), at (7, 37, 41), (33, 10, 9), (1, 5, 7),
# (7, 37, 41) and (198, 12, 9) in PARAMS' order.  Below one fp32 ulp of 1: the sums over t are fp64, so what is
# left is U's own rounding.
MEASURED_U = {(1, 1): 4.8e-8, (3, 3): 4.4e-8, (7, 2): 3.7e-8, (5, 5): 3.7e-8, (7, 5): 3.4e-8}
TOL_U = {k: 4 * v for k, v in MEASURED_U.items()}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lrspnp import _lib, ops
    _lib.device_lib()
    return ops


def _inputs(shape, seed=0):
    """X, L2 (P, B) float32 numpy with Z = X + C2 L2 in [0, 1] up to rounding, and Z as torch computes it."""
    B, H, W = shape
    rng = np.random.default_rng(100 + seed + B + 31 * H + 977 * W)
    z = rng.random((H * W, B)).astype(np.float32)
    L2 = ((rng.random((H * W, B)) - 0.5) * 0.25).astype(np.float32)
    X = (z - np.float32(C2) * L2).astype(np.float32)
    Z = (torch.from_numpy(X) + C2 * torch.from_numpy(L2)).numpy()
    return X, L2, Z


def _d(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(ops, shape, X, L2, ps, pd, h=0.05, sigma=0.0, ws=None):
    B, H, W = shape
    ws = ops.nlmcube_workspace(H, W, B, ps, pd, "cuda") if ws is None else ws
    U = ops.nlmcube(_d(X), _d(L2), C2, H, W, ws, patch_size=ps, patch_distance=pd, h=h, sigma=sigma)
    torch.cuda.synchronize()
    return U.cpu().numpy()


_REF = {}


def _ref(shape, ps, pd, h, sigma):
    """U (P, B) fp64 of the restatement on _inputs(shape)'s Z; computed once per case."""
    key = (shape, ps, pd, h, sigma)
    if key not in _REF:
        B, H, W = shape
        _REF[key] = R.unfolded(R.nlm(R.image(_inputs(shape)[2], H, W), ps, pd, h, sigma))
    return _REF[key]


# ---- 1. bit-exact identities -------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_no_window_returns_z(ops, shape):
    X, L2, Z = _inputs(shape)
    for ps in (1, 3, 5, 7):
        assert np.array_equal(_run(ops, shape, X, L2, ps, 0), Z), ps
        assert np.array_equal(_run(ops, shape, X, None, ps, 0), X), ps


# h = 1e-4 (ih2 = 1e8): every weight but w(p, 0) underflows to 0 on a random cube with a few bands
@pytest.mark.parametrize("shape", [(3, 6, 1), (4, 9, 11), (5, 8, 12), (7, 37, 41), (33, 10, 9), (198, 12, 9)])
def test_tiny_h_returns_z(ops, shape):
    B, H, W = shape
    X, L2, Z = _inputs(shape)
    for ps, pd in PARAMS:
        for x, l2, z in ((X, L2, Z), (X, None, X)):
            assert np.array_equal(R.nlm(R.image(z, H, W), ps, pd, 1e-4, 0.0), R.image(z, H, W))   # the premise, in fp64
            assert np.array_equal(_run(ops, shape, x, l2, ps, pd, h=1e-4), z), (ps, pd)


@pytest.mark.parametrize("ps,pd", PARAMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_constant_cube_is_a_fixed_point(ops, shape, ps, pd):
    B, H, W = shape
    X = np.full((H * W, B), 0.640625, np.float32)
    assert np.array_equal(_run(ops, shape, X, None, ps, pd, h=0.05, sigma=0.0), X)
    # ... and as X + C2 L2 = 0.5 + 0.5 * 0.28125
    X5, L2 = np.full_like(X, 0.5), np.full_like(X, 0.28125)
    assert np.array_equal(_run(ops, shape, X5, L2, ps, pd, h=0.2, sigma=0.05), X)


# ---- 2. a huge sigma: the clipped-window mean ----------------------------------------------------------
@pytest.mark.parametrize("ps,pd", PARAMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_huge_sigma_is_the_clipped_window_mean(ops, shape, ps, pd):
    B, H, W = shape
    X, L2, Z = _inputs(shape)
    want = R.unfolded(R.window_mean(R.image(Z, H, W), pd))
    err = float(np.abs(_run(ops, shape, X, L2, ps, pd, h=0.1, sigma=10.0) - want).max())
    print(f"nlmcube window mean {shape} ({ps}, {pd}): err {err:.3e}")
    assert err <= 4 * ULP1


# ---- 3. parity with the restatement ------------------------------------------------------------------
def _parity(ops, shape, ps, pd, h, sigma):
    X, L2, _ = _inputs(shape)
    U = _run(ops, shape, X, L2, ps, pd, h=h, sigma=sigma)
    Ur = _ref(shape, ps, pd, h, sigma)
    err = float(np.abs(U - Ur).max())
    print(f"nlmcube parity {shape} ({ps}, {pd}) h={h} sigma={sigma}: U err {err:.3e}")
    return err, U, Ur


@pytest.mark.parametrize("ps,pd", PARAMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_parity(ops, shape, ps, pd):
    worst = max(_parity(ops, shape, ps, pd, h, sigma)[0] for h, sigma in H_SIGMA)
    print(f"nlmcube worst {shape} ({ps}, {pd}): U {worst:.3e}")
    assert worst <= TOL_U[(ps, pd)], worst


# ---- 6. many workgroups: the tile seams --------------------------------------------------------------
@pytest.mark.parametrize("ps,pd", [(7, 2), (5, 5)])
def test_many_workgroups_and_tile_seams(ops, ps, pd):
    B, H, W = BIG
    worst = 0.0
    for h, sigma in H_SIGMA:
        err, U, Ur = _parity(ops, BIG, ps, pd, h, sigma)
        worst = max(worst, err)
        u, ur = R.image(U, H, W), R.image(Ur, H, W)
        # the last row / column of a tile and the first of the next, for every seam
        ys = [y for y in range(H) if y % TILE in (0, TILE - 1)]
        xs = [x for x in range(W) if x % TILE in (0, TILE - 1)]
        seam = max(float(np.abs(u[:, ys] - ur[:, ys]).max()), float(np.abs(u[:, :, xs] - ur[:, :, xs]).max()))
        moved = float(np.abs(ur[:, ys] - R.image(_inputs(BIG)[2], H, W)[:, ys]).max())
        print(f"nlmcube seams {BIG} ({ps}, {pd}) h={h} sigma={sigma}: err {seam:.3e}, the prox moved them {moved:.3e}")
        assert seam <= TOL_U[(ps, pd)] and (moved > 1e-3 or h < 0.2)   # (h = 0.05: the weights underflow, U = Z)
    assert worst <= TOL_U[(ps, pd)], worst


# ---- 4. denoising ------------------------------------------------------------------------------------
def test_denoising(ops):
    clean, noisy = R.denoising_case()
    B, H, W = noisy.shape
    X = R.unfolded(noisy).astype(np.float32)
    U = R.image(_run(ops, (B, H, W), X, None, 3, 3, h=0.05, sigma=0.05), H, W)
    mse = lambda a: float(((a - clean) ** 2).mean())   # noqa: E731
    ratio = mse(U.astype(np.float64)) / mse(R.image(X, H, W).astype(np.float64))
    print(f"nlmcube denoising: MSE ratio {ratio:.4f}")
    assert ratio <= 0.3


# ---- 5. determinism ----------------------------------------------------------------------------------
@pytest.mark.parametrize("ps,pd", [(3, 3), (7, 2)])
@pytest.mark.parametrize("shape", [(4, 9, 11), (2, 2, 2), (7, 37, 41), (198, 12, 9)])
def test_reruns_and_a_misaligned_base_give_the_same_bits(ops, shape, ps, pd):
    B, H, W = shape
    X, L2, _ = _inputs(shape)
    U1 = _run(ops, shape, X, L2, ps, pd, h=0.2, sigma=0.02)
    U2 = _run(ops, shape, X, L2, ps, pd, h=0.2, sigma=0.02)
    assert np.array_equal(U1, U2)
    # X and U one float off a 16-byte boundary: the scalar form
    n = H * W * B
    xb = torch.zeros(n + 4, dtype=torch.float32, device="cuda")
    ub = torch.zeros(n + 4, dtype=torch.float32, device="cuda")
    Xm, Um = xb[1:1 + n].view(H * W, B), ub[1:1 + n].view(H * W, B)
    assert Xm.data_ptr() % 16 == 4 and Um.data_ptr() % 16 == 4
    Xm.copy_(_d(X))
    ops.nlmcube(Xm, _d(L2), C2, H, W, ops.nlmcube_workspace(H, W, B, ps, pd, "cuda"), U=Um, patch_size=ps,
                patch_distance=pd, h=0.2, sigma=0.02)
    torch.cuda.synchronize()
    assert np.array_equal(Um.cpu().numpy(), U1)
    assert float(ub[0]) == 0.0 and not ub[1 + n:].any()      # nothing outside U was written


# ---- 7. workspace ------------------------------------------------------------------------------------
def test_a_cold_call_ignores_the_workspace(ops):
    shape = (4, 9, 11)
    B, H, W = shape
    X, L2, _ = _inputs(shape)
    for ps, pd in PARAMS:
        U1 = _run(ops, shape, X, L2, ps, pd, h=0.2)
        ws = ops.nlmcube_workspace(H, W, B, ps, pd, "cuda")
        ws.fill_(255)                                        # NaN bytes, where there are any
        assert np.array_equal(_run(ops, shape, X, L2, ps, pd, h=0.2, ws=ws), U1)
        # more workspace than asked for is ignored too
        ws = torch.full((4096,), 255, dtype=torch.uint8, device="cuda")
        assert np.array_equal(_run(ops, shape, X, L2, ps, pd, h=0.2, ws=ws), U1)


# ---- 8. the solver -----------------------------------------------------------------------------------
def _solver(cfg, image_shape=(12, 10)):
    from lrspnp import LrsPnP
    from lrspnp.data import mask_matrix, synthetic_cube, synthetic_dictionary, unfold
    H, W, B = 12, 10, 8
    obs, _, _ = synthetic_cube(H, W, B, seed=3)
    pix = (np.random.default_rng(0).random((H, W)) > 0.2).astype(np.float32)
    M = mask_matrix(pix, B)
    return LrsPnP(unfold(obs) * M, M, synthetic_dictionary(16, 64, 0), cfg, image_shape=image_shape)


def test_solver_runs_the_nlm_prox(ops):
    from lrspnp import LrsPnPConfig, NlmCubeConfig
    nlm = NlmCubeConfig(3, 2, 0.1, 0.0)
    s = _solver(LrsPnPConfig(lowrank="nlm", nlm=nlm, bb=4, sliding=4))
    ws = ops.nlmcube_workspace(12, 10, 8, 3, 2, "cuda")
    for it in (1, 2):
        X0, L20 = s.X.clone(), s.L2.clone()
        s.step()
        torch.cuda.synchronize()
        direct = ops.nlmcube(X0, L20, s.c2, 12, 10, ws, patch_size=3, patch_distance=2, h=0.1, sigma=0.0)
        torch.cuda.synchronize()
        assert torch.equal(s.U, direct), it
        assert not torch.equal(s.U, X0 + s.c2 * L20), it     # ... and the prox did something
        assert s.iteration == it and all(np.isfinite(s.convergence())), it
    for t in (s.X, s.L1, s.L2, s.U):
        assert bool(torch.isfinite(t).all())
    # the defaults construct and step too
    d = _solver(LrsPnPConfig(lowrank="nlm", bb=4, sliding=4, Nit=10))
    assert (d.nlm.patch_size, d.nlm.patch_distance, d.nlm.h, d.nlm.sigma) == (7, 2, 0.05, 0.0)
    d.step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(d.X).all())


def test_solver_refusals(ops):
    from lrspnp import LrsError, LrsPnPConfig, NlmCubeConfig
    base = dict(lowrank="nlm", bb=4, sliding=4, Nit=10)
    with pytest.raises(LrsError, match="image_shape"):
        _solver(LrsPnPConfig(**base), image_shape=None)
    with pytest.raises(LrsError, match="does not match"):
        _solver(LrsPnPConfig(**base), image_shape=(12, 11))
    for bad in (dict(patch_size=4), dict(patch_distance=6), dict(h=0.0)):
        with pytest.raises(LrsError, match="NlmCubeConfig"):
            _solver(LrsPnPConfig(nlm=NlmCubeConfig(**bad), **base))
    with pytest.raises(LrsError) as e:
        _solver(LrsPnPConfig(bb=4, sliding=4, Nit=10, lowrank="nuclear"))
    assert "nlm" in str(e.value)

"""GPU: the TV prox on the cube (csrc/tvprox.hip: lrs_tvprox_f32, ops.tvprox) and lowrank="tv".

Against tests/tvprox_ref.py (the fp64 restatement of the same fixed iteration): bit-exact identities, the
two-element closed forms, parity of U and of both stats at 1, 2, 3 and 25 iterations, the stats against a host
recomputation and against ops.sstv, determinism (reruns, an aligned and a misaligned base), the workspace and
the warm start, several workgroups, and the solver.

Tolerances.  TOL_U[terms]: the absolute error of U for inputs in [0, 1]; TOL_S[terms]: the error
of either stat as a fraction of the primal objective.  Each is four times the largest error measured on the
MI355X over SHAPES x N_ITERS for that term set, against the fp64 restatement.
"""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tvprox_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 5, 7), (3, 1, 6), (3, 6, 1), (2, 2, 2), (4, 9, 11), (5, 8, 12), (7, 37, 41)]   # (B, H, W)
BIG = (31, 190, 170)
N_ITERS = (1, 2, 3, 25)
f32 = lambda v: float(np.float32(v))   # noqa: E731  (the weights as the library receives them)
TAU = 1.25
# tau w = 0.05 for each weight alone; 0.05, 0.04, 0.06 together
TERMS = {"spatial": (f32(0.04), 0.0, 0.0), "band": (0.0, f32(0.04), 0.0), "sstv": (0.0, 0.0, f32(0.04)),
         "all": (f32(0.04), f32(0.032), f32(0.048))}
C2 = 0.5
# measured maxima (MI355X, SHAPES x N_ITERS, and BIG at 2 iterations), DESIGN §12.  U: (7, 37, 41) at 25 iterations
# (spatial, all) and 3 (band), BIG (sstv): one to two fp32 ulps of 1.  Stats: the smallest shapes, (3, 6, 1) and
# (2, 2, 2), at 1 or 2 iterations, where a rounding of one element of U is the largest share of the objective.
MEASURED_U = {"spatial": 6.7e-8, "band": 6.4e-8, "sstv": 7.9e-8, "all": 1.13e-7}
MEASURED_S = {"spatial": 1.3e-8, "band": 1.8e-8, "sstv": 4.1e-8, "all": 3.5e-8}
TOL_U = {k: 4 * v for k, v in MEASURED_U.items()}
TOL_S = {k: 4 * v for k, v in MEASURED_S.items()}


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


def _run(ops, shape, X, L2, w, tau=TAU, n_iter=0, warm=False, ws=None):
    B, H, W = shape
    ws = ops.tvprox_workspace(H, W, B, "cuda") if ws is None else ws
    stats = torch.full((2,), float("nan"), dtype=torch.float64, device="cuda")
    U = ops.tvprox(_d(X), _d(L2), C2, H, W, ws, w_sp=w[0], w_bd=w[1], w_ss=w[2], tau=tau, n_iter=n_iter, warm=warm,
                   stats=stats)
    torch.cuda.synchronize()
    return U.cpu().numpy(), stats.cpu().numpy(), ws


_REF = {}


def _ref(shape, terms, n_iter, seed=0):
    """(U (P, B), objective, gap, p) of the restatement; computed once per case."""
    key = (shape, terms, n_iter, seed)
    if key not in _REF:
        B, H, W = shape
        _, _, Z = _inputs(shape, seed)
        z, w = R.image(Z, H, W), TERMS[terms]
        U, p = R.fgp(z, *w, tau=TAU, n_iter=n_iter)
        _REF[key] = (R.unfolded(U), R.objective(U, z, *w, tau=TAU), R.gap(U, p, *w, tau=TAU), p)
    return _REF[key]


# ---- 1. bit-exact identities -------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_no_term_no_tau_no_iteration_return_z(ops, shape):
    X, L2, Z = _inputs(shape)
    w = TERMS["all"]
    for kw in (dict(w=(0.0, 0.0, 0.0), n_iter=5), dict(w=w, tau=0.0, n_iter=5), dict(w=w, n_iter=0)):
        U, st, _ = _run(ops, shape, X, L2, **kw)
        assert np.array_equal(U, Z), kw
        if kw["n_iter"]:
            assert st.tolist() == [0.0, 0.0], kw
        else:   # the pair (Z, p = 0): objective = gap = tau T(Z)
            B, H, W = shape
            want = TAU * R.regulariser(R.image(Z, H, W), *w)
            assert abs(st[0] - want) <= 1e-12 * want and st[1] >= 0 and abs(st[1] - want) <= 1e-6 * want, (st, want)
    U, _, _ = _run(ops, shape, X, None, w=w, n_iter=0)
    assert np.array_equal(U, X)


@pytest.mark.parametrize("terms", list(TERMS))
@pytest.mark.parametrize("shape", SHAPES)
def test_constant_cube_is_a_fixed_point(ops, shape, terms):
    B, H, W = shape
    X = np.full((H * W, B), 0.640625, np.float32)
    U, st, _ = _run(ops, shape, X, None, TERMS[terms], n_iter=4)
    assert np.array_equal(U, X) and st.tolist() == [0.0, 0.0]


@pytest.mark.parametrize("shape", SHAPES)
def test_sstv_alone_ignores_separable_cubes(ops, shape):
    """a[c] + b[y, x] on multiples of 2^-6: every second difference is exactly 0, so U == Z under w_ss alone."""
    B, H, W = shape
    rng = np.random.default_rng(4)
    a = rng.integers(0, 128, size=(B, 1, 1)) / 64.0
    b = rng.integers(0, 128, size=(1, H, W)) / 64.0
    X = R.unfolded((a + b).astype(np.float32))
    U, st, _ = _run(ops, shape, X, None, TERMS["sstv"], n_iter=6)
    assert np.array_equal(U, X) and st.tolist() == [0.0, 0.0]


# ---- 2. closed forms ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,unit,lip", [((2, 1, 1), (0.0, 1.0, 0.0), 4.0), ((1, 2, 1), (1.0, 0.0, 0.0), 8.0),
                                            ((1, 1, 2), (1.0, 0.0, 0.0), 8.0)])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_two_elements_saturate(ops, shape, unit, lip, sign):
    z0, d = 0.375, sign * 0.5
    z = np.array([z0, z0 + d], np.float32).reshape(shape)
    ulp = float(np.spacing(np.float32(np.abs(z).max())))
    for tw in (0.5 / lip, 0.03125):
        w = tuple(0.25 * v for v in unit)
        for n in (1, 2, 7):
            U, _, _ = _run(ops, shape, R.unfolded(z), None, w, tau=4.0 * tw, n_iter=n)
            want = np.array([z0 + sign * tw, z0 + d - sign * tw])
            assert np.abs(R.image(U, shape[1], shape[2]).reshape(-1) - want).max() <= ulp, (tw, n)


# ---- 3. parity with the restatement; 4. stats --------------------------------------------------------
def _parity(ops, shape, terms, n_iter):
    X, L2, Z = _inputs(shape)
    w = TERMS[terms]
    U, st, _ = _run(ops, shape, X, L2, w, n_iter=n_iter)
    Ur, obj, gap, _ = _ref(shape, terms, n_iter)
    eu = float(np.abs(U - Ur).max())
    es = max(abs(st[0] - obj), abs(st[1] - gap)) / obj if obj > 0 else max(abs(st[0]), abs(st[1]))
    print(f"tvprox parity {shape} {terms} n={n_iter}: U err {eu:.3e}, stats err {es:.3e} of obj {obj:.6e}, "
          f"gap {st[1]:.3e} (ref {gap:.3e})")
    return eu, es, U, st, Z, obj


@pytest.mark.parametrize("terms", list(TERMS))
@pytest.mark.parametrize("shape", SHAPES)
def test_parity_and_stats(ops, shape, terms):
    B, H, W = shape
    w = TERMS[terms]
    worst_u = worst_s = 0.0
    checks = []
    for n in N_ITERS:
        eu, es, U, st, Z, obj = _parity(ops, shape, terms, n)
        worst_u, worst_s = max(worst_u, eu), max(worst_s, es)
        # the objective recomputed in fp64 on the host from the returned U
        host = R.objective(R.image(U, H, W), R.image(Z, H, W), *w, tau=TAU)
        # ... and through the other definition of the operators, lrs_sstv_f32
        img = ops.unfolded_to_image(_d(U), None, 1.0, H, W)
        T, _ = ops.sstv(img, spatial=w[0], band=w[1], sstv=w[2], eps=0.0, n_mean=1)
        fid = 0.5 * float(((_d(U).double() - _d(Z).double()) ** 2).sum())
        cross = fid + TAU * float(T)
        print(f"   stats[0] {st[0]:.9e} host {host:.9e} via sstv {cross:.9e}")
        checks.append((n, st, host, cross, obj))
    print(f"tvprox worst {shape} {terms}: U {worst_u:.3e} stats {worst_s:.3e}")
    assert worst_u <= TOL_U[terms] and worst_s <= TOL_S[terms], (worst_u, worst_s)
    for n, st, host, cross, obj in checks:
        assert np.isfinite(st).all() and st[1] >= -TOL_S[terms] * obj, (n, st)
        assert abs(st[0] - host) <= 1e-6 * host, (n, st[0], host)
        assert abs(st[0] - cross) <= 1e-5 * cross, (n, st[0], cross)


@pytest.mark.parametrize("terms", ["sstv", "all"])
def test_many_workgroups(ops, terms):
    eu, es, _, st, _, obj = _parity(ops, BIG, terms, 2)
    assert eu <= TOL_U[terms] and es <= TOL_S[terms] and st[1] >= -TOL_S[terms] * obj, (eu, es, st)


# ---- 5. determinism ----------------------------------------------------------------------------------
@pytest.mark.parametrize("terms", ["sstv", "all"])
@pytest.mark.parametrize("shape", [(4, 9, 11), (2, 2, 2), (7, 37, 41)])
def test_reruns_and_a_misaligned_base_give_the_same_bits(ops, shape, terms):
    B, H, W = shape
    X, L2, _ = _inputs(shape)
    w = TERMS[terms]
    U1, s1, _ = _run(ops, shape, X, L2, w, n_iter=5)
    U2, s2, _ = _run(ops, shape, X, L2, w, n_iter=5)
    assert np.array_equal(U1, U2) and np.array_equal(s1, s2)
    # X and U one float off a 16-byte boundary: the scalar form
    n = H * W * B
    xb = torch.zeros(n + 4, dtype=torch.float32, device="cuda")
    ub = torch.zeros(n + 4, dtype=torch.float32, device="cuda")
    Xm, Um = xb[1:1 + n].view(H * W, B), ub[1:1 + n].view(H * W, B)
    assert Xm.data_ptr() % 16 == 4 and Um.data_ptr() % 16 == 4
    Xm.copy_(_d(X))
    st = torch.zeros(2, dtype=torch.float64, device="cuda")
    ops.tvprox(Xm, _d(L2), C2, H, W, ops.tvprox_workspace(H, W, B, "cuda"), U=Um, w_sp=w[0], w_bd=w[1], w_ss=w[2],
               tau=TAU, n_iter=5, stats=st)
    torch.cuda.synchronize()
    assert np.array_equal(Um.cpu().numpy(), U1) and np.array_equal(st.cpu().numpy(), s1)


# ---- 6. workspace and warm start ---------------------------------------------------------------------
def test_a_cold_call_ignores_the_workspace(ops):
    shape = (4, 9, 11)
    B, H, W = shape
    X, L2, _ = _inputs(shape)
    U1, s1, _ = _run(ops, shape, X, L2, TERMS["all"], n_iter=4)
    ws = ops.tvprox_workspace(H, W, B, "cuda")
    ws[: ws.numel() // 4 * 4].view(torch.float32).fill_(float("nan"))
    U2, s2, _ = _run(ops, shape, X, L2, TERMS["all"], n_iter=4, ws=ws)
    assert np.array_equal(U1, U2) and np.array_equal(s1, s2)


@pytest.mark.parametrize("terms", list(TERMS))
def test_warm_start_continues(ops, terms):
    """A warm call is the restatement started from the previous call's p: 3 cold + 2 warm iterations."""
    shape = (5, 8, 12)
    B, H, W = shape
    X, L2, Z = _inputs(shape)
    w = TERMS[terms]
    _, _, ws = _run(ops, shape, X, L2, w, n_iter=3)
    U, st, _ = _run(ops, shape, X, L2, w, n_iter=2, warm=True, ws=ws)
    z = R.image(Z, H, W)
    Ur, pr = R.fgp(z, *w, tau=TAU, n_iter=2, p0=_ref(shape, terms, 3)[3])
    obj, gap = R.objective(Ur, z, *w, tau=TAU), R.gap(Ur, pr, *w, tau=TAU)
    eu = float(np.abs(U - R.unfolded(Ur)).max())
    es = max(abs(st[0] - obj), abs(st[1] - gap)) / obj
    print(f"tvprox warm {terms}: U err {eu:.3e}, stats err {es:.3e}")
    assert eu <= TOL_U[terms] and es <= TOL_S[terms]


# (shape, terms) at which 300 iterations of the restatement have converged to far below fp32 resolution: one more
# warm iteration moves its U by less than 1e-9 (checked below on the restatement itself, before the GPU runs)
WARM_CONVERGED = [((2, 2, 2), "all"), ((1, 5, 7), "spatial"), ((3, 1, 6), "band")]


@pytest.mark.parametrize("shape,terms", WARM_CONVERGED)
def test_warm_start_at_the_solution_stays(ops, shape, terms):
    B, H, W = shape
    X, L2, Z = _inputs(shape)
    w = TERMS[terms]
    z = R.image(Z, H, W)
    Ur, pr = R.fgp(z, *w, tau=TAU, n_iter=300)
    Ur1, _ = R.fgp(z, *w, tau=TAU, n_iter=1, p0=pr)
    assert np.abs(Ur1 - Ur).max() < 1e-9      # the premise, in fp64
    U300, _, ws = _run(ops, shape, X, L2, w, n_iter=300)
    U1, st, _ = _run(ops, shape, X, L2, w, n_iter=1, warm=True, ws=ws)
    move = float(np.abs(U1 - U300).max())
    print(f"tvprox warm at the solution {shape} {terms}: moved {move:.3e}")
    assert move <= TOL_U[terms] and np.isfinite(st).all()


@pytest.mark.parametrize("terms", list(TERMS))
def test_warm_start_clips_to_smaller_radii(ops, terms):
    """tau halved between the calls: the p left behind exceeds the new radii and is clipped, which the gap shows
    (it has a term r |d| - p d per difference, negative as soon as |p| > r where p and d agree in sign)."""
    shape = (4, 9, 11)
    X, L2, _ = _inputs(shape)
    w = TERMS[terms]
    _, _, ws = _run(ops, shape, X, L2, w, n_iter=30)
    _, st, _ = _run(ops, shape, X, L2, w, tau=TAU / 2, n_iter=1, warm=True, ws=ws)
    print(f"tvprox warm, tau halved, {terms}: stats {st}")
    assert np.isfinite(st).all() and st[0] > 0 and st[1] >= -TOL_S[terms] * st[0]


# ---- 7. the solver -----------------------------------------------------------------------------------
def _solver(cfg, image_shape=(12, 10)):
    from lrspnp import LrsPnP
    from lrspnp.data import mask_matrix, synthetic_cube, synthetic_dictionary, unfold
    H, W, B = 12, 10, 8
    obs, _, _ = synthetic_cube(H, W, B, seed=3)
    pix = (np.random.default_rng(0).random((H, W)) > 0.2).astype(np.float32)
    M = mask_matrix(pix, B)
    return LrsPnP(unfold(obs) * M, M, synthetic_dictionary(16, 64, 0), cfg, image_shape=image_shape)


def test_solver_runs_the_tv_prox(ops):
    from lrspnp import LrsPnPConfig, TvProxConfig
    tv = TvProxConfig(w_sp=0.02, w_bd=0.01, w_ss=0.05, n_iter=7)
    s = _solver(LrsPnPConfig(bb=4, sliding=4, Nit=10, lowrank="tv", tv=tv))
    X0, L20 = s.X.clone(), s.L2.clone()
    s.step()
    torch.cuda.synchronize()
    U = s.U.clone()
    ws = ops.tvprox_workspace(12, 10, 8, "cuda")
    direct = ops.tvprox(X0, L20, s.c2, 12, 10, ws, w_sp=tv.w_sp, w_bd=tv.w_bd, w_ss=tv.w_ss, tau=s.tau, n_iter=tv.n_iter)
    torch.cuda.synchronize()
    assert torch.equal(U, direct)
    s.step()
    torch.cuda.synchronize()
    assert s.iteration == 2
    for t in (s.X, s.L1, s.L2, s.U):
        assert bool(torch.isfinite(t).all())
    # the defaults construct and step too
    d = _solver(LrsPnPConfig(bb=4, sliding=4, Nit=10, lowrank="tv"))
    assert (d.tv.w_sp, d.tv.w_bd, d.tv.w_ss, d.tv.n_iter, d.tv.warm) == (0.0, 0.0, 1.0, 20, True)
    d.step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(d.X).all())


def test_solver_refusals(ops):
    from lrspnp import LrsError, LrsPnPConfig
    with pytest.raises(LrsError, match="image_shape"):
        _solver(LrsPnPConfig(bb=4, sliding=4, Nit=10, lowrank="tv"), image_shape=None)
    with pytest.raises(LrsError, match="does not match"):
        _solver(LrsPnPConfig(bb=4, sliding=4, Nit=10, lowrank="tv"), image_shape=(12, 11))
    with pytest.raises(LrsError) as e:
        _solver(LrsPnPConfig(bb=4, sliding=4, Nit=10, lowrank="nuclear"))
    for name in ("svt", "dip", "tv"):
        assert name in str(e.value)

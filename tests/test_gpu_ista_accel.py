"""Accelerated (FISTA) sparse coding, lrs_ista_opts.accel = LRS_ISTA_ACCEL_FISTA, on a real MI355X
against the float32 restatement tests/fista_ref.py (which is oracle.ista_batch bit for bit when the
momentum is off: tests/test_fista_ref.py).

Tolerance: the project's bar for the sparse-coding kernels, 1e-5 relative L2 per block on the
coefficients and on Phi; for the MATLAB prox max(1e-5, 4 x sens), sens being the restatement's own
change under a 1-ulp perturbation of Yb (as test_gpu_kernels.py::test_ista_kernel_vs_oracle).
Data: that test's helper (20 % missing, one fully observed block, one half-masked block); the
per-pattern cases use its _pattern_case.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import dictlearn_ref as R  # noqa: E402
import fista_ref as F  # noqa: E402
from oracle import oracle as O  # noqa: E402
from test_gpu_kernels import _pattern_case  # noqa: E402

pytestmark = pytest.mark.gpu

# (bb, nb, Nit, variant, K)
RS_CASES = [(36, 20, 12, "fro4", 256), (36, 17, 10, "fro4", 512), (36, 23, 8, "spec2", 200),
            (8, 33, 20, "spec2", 100), (8, 21, 10, "fro4", 7), (20, 37, 10, "soft", 256),
            (36, 30, 30, "soft", 256), (36, 5, 8, "matlab", 256), (36, 250, 5, "fro4", 256)]
RESIDENT_CASES = [(8, 70, 30, "soft", 256), (8, 129, 20, "fro4", 256)]
GENERIC_CASES = [(36, 21, 10, "fro4", 768), (8, 40, 12, "soft", 1024)]
# (bb, nb, Nit, variant, K, npat)
PAT_CASES = [(36, 40, 12, "fro4", 256, 3), (36, 21, 8, "soft", 256, 2), (36, 18, 8, "fro4", 512, 2),
             (8, 40, 10, "fro4", 7, 3), (36, 70, 1, "fro4", 256, 3)]


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


def worst(a, b):
    return max(rel(a[j], b[j]) for j in range(len(b)))


_cases = {}


def case(bb, nb, Nit, variant, K):
    """Inputs, the accelerated restatement and its tolerance for one shape, computed once."""
    key = (bb, nb, Nit, variant, K)
    if key not in _cases:
        D, Yb, obs, alpha, thr, prox = F.case(bb, nb, variant, K, bb * 1000 + nb + K)
        X, PHI = F.ista(Yb, obs, D, alpha, thr, Nit, prox, accel=True)
        tol = 1e-5
        if variant == "matlab" and Nit > 1:
            rng = np.random.default_rng(bb + nb + K)
            flip = np.where(rng.random(Yb.shape) < 0.5, -1.0, 1.0)
            Yp = (Yb.astype(np.float64) * (1.0 + flip * 2.0 ** -23)).astype(np.float32)
            Xp, PHIp = F.ista(Yp, obs, D, alpha, thr, Nit, prox, accel=True)
            tol = max(1e-5, 4.0 * max(worst(Xp, X), worst(PHIp, PHI)))
        _cases[key] = (D, Yb, obs, alpha, thr, prox, X, PHI, tol)
    return _cases[key]


def run(ops, D, Yb, obs, alpha, thr, Nit, prox, **kw):
    """ops.ista on the padded blocks; returns (phi[:, :n], coefs) as numpy, the pad checked zero."""
    n = D.shape[0]
    n_pad = -(-n // 16) * 16
    pad = lambda a: np.pad(a, ((0, 0), (0, n_pad - n)))
    phi, coefs = ops.ista(d(pad(Yb)), d(pad(obs)), d(D), n, d(alpha), d(thr), Nit, prox, want_coefs=True, **kw)
    phi = phi.cpu().numpy()
    assert np.all(phi[:, n:] == 0)
    return phi[:, :n], coefs.cpu().numpy()


def check(name, phi, coefs, X, PHI, tol):
    ec, ep = worst(coefs, X), worst(phi, PHI)
    print(f"{name}: coefs {ec:.3e}, phi {ep:.3e} (tol {tol:.1e})")
    assert ec < tol, (ec, tol)
    assert ep < tol, (ep, tol)


# ------------------------------------------------------------------------------- the three paths
@pytest.mark.parametrize("bb,nb,Nit,variant,K", RS_CASES)
def test_row_split_vs_restatement(ops, bb, nb, Nit, variant, K):
    D, Yb, obs, alpha, thr, prox, X, PHI, tol = case(bb, nb, Nit, variant, K)
    phi, coefs = run(ops, D, Yb, obs, alpha, thr, Nit, prox, accel="fista")
    check(f"row-split {(bb, nb, Nit, variant, K)}", phi, coefs, X, PHI, tol)


@pytest.mark.parametrize("bb,nb,Nit,variant,K", RESIDENT_CASES)
def test_resident_sizes_run_the_row_split_kernel(ops, bb, nb, Nit, variant, K):
    """n_pad <= 64 with K = 256: the resident kernels have no momentum, so the call is rerouted; its
    result is the restatement's and not the plain iteration's (more than 1e-3 apart over all blocks)."""
    D, Yb, obs, alpha, thr, prox, X, PHI, tol = case(bb, nb, Nit, variant, K)
    assert ops.ista_workspace(bb * bb, K, prox, "cuda") is None
    assert ops.ista_workspace(bb * bb, K, prox, "cuda", accel="fista") is not None
    phi, coefs = run(ops, D, Yb, obs, alpha, thr, Nit, prox, accel="fista")
    check(f"rerouted {(bb, nb, Nit, variant, K)}", phi, coefs, X, PHI, tol)
    phi0, coefs0 = run(ops, D, Yb, obs, alpha, thr, Nit, prox)
    diff = rel(coefs, coefs0)
    print(f"accelerated vs plain coefficients: {diff:.3e}")
    assert diff > 1e-3


@pytest.mark.parametrize("bb,nb,Nit,variant,K", GENERIC_CASES)
def test_generic_path_vs_restatement(ops, bb, nb, Nit, variant, K):
    D, Yb, obs, alpha, thr, prox, X, PHI, tol = case(bb, nb, Nit, variant, K)
    phi, coefs = run(ops, D, Yb, obs, alpha, thr, Nit, prox, accel="fista")
    check(f"generic {(bb, nb, Nit, variant, K)}", phi, coefs, X, PHI, tol)


def test_generic_algorithm_agrees_with_fused_kernel(ops):
    """LRS_ISTA_ALGO_GENERIC at a size the row-split kernel serves: both against the restatement and
    against each other."""
    bb, nb, Nit, variant, K = 36, 12, 6, "soft", 100
    D, Yb, obs, alpha, thr, prox, X, PHI, tol = case(bb, nb, Nit, variant, K)
    phi_g, co_g = run(ops, D, Yb, obs, alpha, thr, Nit, prox, accel="fista", algorithm=1)
    check("generic (36, 12, 6, soft, 100)", phi_g, co_g, X, PHI, tol)
    phi_f, co_f = run(ops, D, Yb, obs, alpha, thr, Nit, prox, accel="fista")
    check("fused (36, 12, 6, soft, 100)", phi_f, co_f, X, PHI, tol)
    assert worst(co_g, co_f) < tol and worst(phi_g, phi_f) < tol


@pytest.mark.parametrize("bb,nb,Nit,variant,K,npat", PAT_CASES)
def test_per_pattern_kernel_vs_restatement(ops, bb, nb, Nit, variant, K, npat):
    """lrs_ista_pat_f32 with accel against the restatement and the accelerated row-split kernel."""
    _, n, D, Yb, obs, alpha, thr, prox, args, dd, pad = _pattern_case(ops, bb, nb, Nit, variant, K, npat,
                                                                      bb * 7 + nb + K + npat)
    X, PHI = F.ista(Yb, obs, D, alpha, thr, Nit, prox, accel=True)
    phi, coefs = ops.ista_pat(**args, want_coefs=True, accel="fista")
    assert np.all(phi.cpu().numpy()[:, n:] == 0)
    phi, coefs = phi.cpu().numpy()[:, :n], coefs.cpu().numpy()
    check(f"per-pattern {(bb, nb, Nit, variant, K, npat)}", phi, coefs, X, PHI, 1e-5)
    phr, cor = ops.ista(args["Yb"], dd(pad(obs)), dd(D), n, args["alpha"], args["thr"], Nit, prox, want_coefs=True,
                        accel="fista")
    assert worst(coefs, cor.cpu().numpy()) < 1e-5
    assert worst(phi, phr.cpu().numpy()[:, :n]) < 1e-5


# ------------------------------------------------------------------------------------------ edges
def _fused_calls(ops):
    """(name, call(Nit, **kw) -> (phi, coefs) device tensors) for the two fused kernels."""
    D, Yb, obs, alpha, thr, prox = F.case(36, 16 * 2 + 5, "fro4", 256, 77)
    base = (d(Yb), d(obs), d(D), D.shape[0], d(alpha), d(thr))
    rs = lambda Nit, **kw: ops.ista(*base, Nit, prox, want_coefs=True, **kw)
    _, _, _, _, _, _, _, _, args, _, _ = _pattern_case(ops, 36, 16 * 2 + 7, 12, "fro4", 256, 3, 91)
    a = {k: v for k, v in args.items() if k != "Nit"}
    pat = lambda Nit, **kw: ops.ista_pat(**a, Nit=Nit, want_coefs=True, **kw)
    return [("row-split", rs), ("per-pattern", pat)]


def test_first_two_iterations_are_plain_ista(ops):
    """beta_1 = 0 and the last iteration writes x itself: Nit 1 and 2 are the plain kernel's bits; the
    third iteration is the first that differs."""
    for name, call in _fused_calls(ops):
        for Nit in (1, 2):
            pa, ca = call(Nit, accel="fista")
            pp, cp = call(Nit)
            assert torch.equal(pa, pp) and torch.equal(ca, cp), (name, Nit)
        assert not torch.equal(call(3, accel="fista")[1], call(3)[1]), name


def test_grid_bound_and_repeat_are_bitwise(ops):
    for name, call in _fused_calls(ops):
        p0, c0 = call(9, accel="fista")
        p1, c1 = call(9, accel="fista", max_workgroups=2)
        p2, c2 = call(9, accel="fista")
        assert torch.equal(p0, p1) and torch.equal(c0, c1), name
        assert torch.equal(p0, p2) and torch.equal(c0, c2), name


def test_zero_iterations_return_the_start(ops):
    D, Yb, obs, alpha, thr, prox = F.case(36, 21, "fro4", 200, 13)
    n, K = D.shape
    base = (d(Yb), d(obs), d(D), n, d(alpha), d(thr))
    phi, coefs = ops.ista(*base, 0, prox, want_coefs=True, accel="fista")
    assert not phi.any() and not coefs.any()
    x0 = (np.random.default_rng(2).standard_normal((21, K)) * 0.1).astype(np.float32)
    co = d(x0)
    phi, _ = ops.ista(*base, 0, prox, coefs=co, want_coefs=True, warm_start=True, accel="fista")
    assert np.array_equal(co.cpu().numpy(), x0)
    ref = x0.astype(np.float64) @ D.astype(np.float64).T
    assert worst(phi.cpu().numpy()[:, :n], ref) < 1e-6
    phi, coefs = ops.ista(*base, 0, prox, want_coefs=True, accel="fista", algorithm=1)
    assert not phi.any() and not coefs.any()


def test_invalid_accel_value_is_refused(ops):
    from lrspnp import _lib
    from lrspnp._lib import LrsError
    L = _lib.device_lib()
    D, Yb, obs, alpha, thr, prox = F.case(8, 20, "fro4", 100, 3)
    n, K = D.shape
    t = [d(Yb), d(obs), d(D), d(alpha), d(thr), torch.zeros((20, 64), device="cuda")]
    ws = ops.ista_workspace(n, K, prox, "cuda")
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    for accel, want in ((2, -1), (-1, -1)):
        o = _lib.ista_opts(accel=accel)
        rc = L.lrs_ista_f32(p(t[0]), p(t[1]), p(t[2]), n, 64, K, 20, p(t[3]), p(t[4]), 3, prox, None, p(t[5]),
                            ctypes.byref(o), p(ws), ws.numel(), None)
        assert rc == want, (accel, rc)
    _, _, _, _, _, _, _, _, args, _, _ = _pattern_case(ops, 8, 20, 3, "fro4", 7, 2, 5)
    o = _lib.ista_opts(accel=2)
    phi = torch.zeros((20, 64), device="cuda")
    rc = L.lrs_ista_pat_f32(p(args["Yb"]), p(args["obs_pat"]), 2, p(args["plan"]), args["ntiles"], 64, 64, 7, 20,
                            p(args["alpha"]), p(args["thr"]), 3, prox, None, p(phi), ctypes.byref(o), p(args["ws"]),
                            args["ws"].numel(), None)
    assert rc == -1
    torch.cuda.synchronize()
    assert not t[5].any() and not phi.any()                  # nothing was launched
    with pytest.raises(LrsError):
        ops.ista(t[0], t[1], t[2], n, t[3], t[4], 3, prox, accel="nesterov")


def test_soft_objective_not_above_ista_on_the_device(ops):
    """||m .* (y - D x)||^2 + lambda ||x||_1 per block of the device's coefficients: FISTA <= ISTA at
    the same Nit (1e-6 relative allowance where both have converged), on all three paths."""
    for bb, nb, Nit, variant, K in [c for c in RS_CASES + RESIDENT_CASES + GENERIC_CASES if c[3] == "soft"]:
        D, Yb, obs, alpha, thr, prox = case(bb, nb, Nit, variant, K)[:6]
        _, ca = run(ops, D, Yb, obs, alpha, thr, Nit, prox, accel="fista")
        _, cp = run(ops, D, Yb, obs, alpha, thr, Nit, prox)
        fa, fp = F.lasso_objective(Yb, obs, D, ca, 0.1), F.lasso_objective(Yb, obs, D, cp, 0.1)
        print(f"device lasso objective {(bb, nb, Nit, K)}: mean FISTA {fa.mean():.6g}, ISTA {fp.mean():.6g}")
        assert np.all(fa <= fp * (1 + 1e-6)), (bb, nb, Nit, K)


# ------------------------------------------------------------------------------------- warm start
@pytest.mark.parametrize("bb,K,variant", [(36, 256, "fro4"), (8, 256, "soft")])
def test_warm_start_restarts_the_momentum(ops, bb, K, variant):
    """accel with warm_start: from the given coefficients with t = 1 and x_prev = x0, i.e. the
    restatement started at x0 (not the continuation of a longer call).  bb = 8 with K = 256: a size
    whose plain call refuses warm_start, served by the row-split kernel under accel."""
    from lrspnp._lib import LrsError
    nb, Nit = 19, 7
    D, Yb, obs, alpha, thr, prox = F.case(bb, nb, variant, K, 31 + bb)
    x0, _ = F.ista(Yb, obs, D, alpha, thr, 4, prox, accel=True)
    X, PHI = F.ista(Yb, obs, D, alpha, thr, Nit, prox, accel=True, x0=x0)
    co = d(x0)
    phi, coefs = run(ops, D, Yb, obs, alpha, thr, Nit, prox, accel="fista", warm_start=True, coefs=co)
    check(f"warm start bb {bb}", phi, coefs, X, PHI, 1e-5)
    if bb == 8:
        with pytest.raises(LrsError):
            run(ops, D, Yb, obs, alpha, thr, Nit, prox, warm_start=True, coefs=d(x0))


# ----------------------------------------------------------------------------------------- solver
@pytest.mark.parametrize("variant", ["spec2", "soft"])
def test_solver_step_uses_the_accelerated_call(ops, golden, variant):
    """One LrsPnP.step() with ista_accel='fista' on the native 36 x 36 x 128 data: Phi is that of the
    matching accelerated ops call on the step's blocks, and not the plain call's."""
    from lrspnp import LrsPnP, LrsPnPConfig
    from lrspnp.data import mask_matrix, synthetic_dictionary, unfold
    g = golden("data_img5.npz")
    Y, M = unfold(g["noisy_img5"][0]), mask_matrix(g["fourth_mask"], 128)
    D = synthetic_dictionary(1296, 256, 0)
    s = LrsPnP(Y, M, D, LrsPnPConfig(bb=36, sliding=36, Nit=12, variant=variant, ista_accel="fista"))
    s.step()
    torch.cuda.synchronize()
    phi = s.phi.clone()
    out = {}
    for accel in ("fista", "off"):
        if s.pat_plan is not None:
            out[accel] = ops.ista_pat(s.Yb, s.obs_pat, s.pat_plan, s.pat_ntiles, s.K, s.n, s.alpha, s.thr, 12,
                                      s.ista_ws, s.prox, accel=accel)
        else:
            out[accel] = ops.ista(s.Yb, s.obs, s.D, s.n, s.alpha, s.thr, 12, s.prox, accel=accel)
    assert torch.equal(phi, out["fista"])
    assert not torch.equal(phi, out["off"])
    assert torch.isfinite(s.X).all()


def test_solver_refuses_sliced_accelerated_coding(ops):
    from lrspnp import LrsPnP, LrsPnPConfig
    from lrspnp._lib import LrsError
    from lrspnp.data import mask_matrix, synthetic_cube, synthetic_dictionary, unfold
    cube, _, mask = synthetic_cube(24, 24, 40, seed=1)
    Y, M, D = unfold(cube), mask_matrix(mask, 40), synthetic_dictionary(64, 64, 0)
    with pytest.raises(LrsError):
        LrsPnP(Y, M, D, LrsPnPConfig.dip_1lip(bb=8, sliding=8, Nit=10, ista_accel="fista", ista_slices_dip=2),
               image_shape=(24, 24))
    with pytest.raises(LrsError):
        LrsPnP(Y, M, D, LrsPnPConfig(bb=8, sliding=8, Nit=10, ista_accel="nesterov"))


# ---------------------------------------------------------------------------- dictionary learning
def test_learn_dictionary_accelerated(ops):
    """learn_blocks with accel='fista' on test_gpu_dictlearn.py's planted problem against the rounds
    assembled from fista_ref.ista (warm start between rounds, momentum restarted) and
    dictlearn_ref.dict_step; that file's end-to-end bar (last objective within 1e-4 relative), and
    the objective never rises inside a dictionary step."""
    from lrspnp.dictlearn import DictLearnConfig, learn_blocks, warm_start_supported
    Y, obs, Ds, D0 = R.planted_problem()
    rounds, Nit, n_inner, lam = 8, 50, 10, 0.1
    cfg = DictLearnConfig(K=32, bb=8, lambda_ista=lam, Nit=Nit, rounds=rounds, n_inner=n_inner, accel="fista")
    assert warm_start_supported(64, 256, False, "fista") and not warm_start_supported(64, 256, False)
    Dr, A = np.array(D0, np.float64), None
    href = np.empty((rounds, n_inner + 1))
    for r in range(rounds):
        alpha, thr = R.ista_alpha_soft(Dr, obs, lam)
        A, _ = F.ista(Y, obs, Dr, alpha, thr, Nit, O.PROX_SOFT, accel=True, x0=A)
        Dr, href[r] = R.dict_step(Y, obs, A, Dr, n_inner)
    D, hist = learn_blocks(d(Y), d(obs), 64, d(D0), cfg)
    hist = hist.cpu().numpy()
    gap = abs(hist[-1, -1] - href[-1, -1]) / href[-1, -1]
    print(f"accelerated planted: objective {hist[0, 0]:.6g} -> {hist[-1, -1]:.6g} (restatement {href[-1, -1]:.6g}, "
          f"rel gap {gap:.3e})")
    assert hist.shape == (rounds, n_inner + 1) and np.isfinite(hist).all()
    assert gap <= max(1e-4, 10 * 7.4e-9)
    assert np.all(hist[:, 1:] <= hist[:, :-1] * (1 + 1e-6))
    assert np.allclose(np.linalg.norm(D.cpu().numpy().astype(np.float64), axis=0), 1.0, atol=1e-6)

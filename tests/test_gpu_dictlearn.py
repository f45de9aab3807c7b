"""Masked dictionary learning on a real MI355X against the fp64 checker (tests/dictlearn_ref.py).

Tolerances (DESIGN.md §8 holds the measurements behind them):
  * dict_stats          : H to 1e-5 of max|H| (the project's ISTA tolerance), c to 1e-6 relative.
  * dict_update, 1 it.  : D to 1e-5 of max|D|, obj to 1e-5 relative.
  * dict_update, 10 it. : four times the checker's own float32-versus-fp64 deviation on these inputs
                          (measured on the CPU: D 1.9e-7 .. 3.2e-7 of max|D|, obj 2.0e-8 .. 7.9e-8
                          relative), and no tighter than 1e-5: so 1e-5 for both.
  * monotonicity        : obj[i+1] <= obj[i] (1 + 1e-6); the float32 checker stays inside it (its
                          largest ratio on these inputs is 0.947, as the fp64 one's).
  * end to end          : last objective within max(1e-4, 10 x 7.4e-9) = 1e-4 relative of the fp64
                          checker's (7.4e-9 = the checker's float32-versus-fp64 gap on the planted
                          problem; the floor because soft-threshold supports may differ).
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import dictlearn_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

STATS_SHAPES = [(37, 48), (1, 256), (1000, 256), (50, 512)]                       # (nb, K)
UPDATE_SHAPES = [(64, 64, 256, 200), (100, 112, 48, 37), (1296, 1296, 256, 50), (1296, 1296, 512, 20)]  # n, n_pad, K, nb


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lrspnp import ops as _ops
    return _ops


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_cache = {}


def update_case(shape):
    """Inputs and the fp64 references (1 and 10 iterations) of one shape, computed once."""
    if shape not in _cache:
        n, n_pad, K, nb = shape
        Yb, ob, A, D = R.update_problem(n, n_pad, K, nb, 100 + UPDATE_SHAPES.index(shape))
        ref = {ni: R.dict_step(Yb[:, :n], ob[:, :n], A, D, ni) for ni in (1, 10)}
        _cache[shape] = (Yb, ob, A, D, ref)
    return _cache[shape]


def run_update(ops, shape, n_inner):
    """dict_stats + dict_update on the device, the workspace poisoned with NaN beforehand."""
    n, n_pad, K, nb = shape
    Yb, ob, A, D, _ = update_case(shape)
    ws = ops.dict_workspace(n, n_pad, K, nb, "cuda")
    ws.view(torch.float32).fill_(float("nan"))
    coefs, Dd = d(A), d(D)
    _, c = ops.dict_stats(coefs, ws=ws)
    ws.view(torch.float32).fill_(float("nan"))
    obj = ops.dict_update(d(Yb), d(ob), coefs, Dd, n, c, n_inner, ws=ws)
    return Dd.cpu().numpy(), obj.cpu().numpy(), float(c.cpu()[0])


@pytest.mark.parametrize("nb,K", STATS_SHAPES)
def test_dict_stats_vs_fp64(ops, nb, K):
    rng = np.random.default_rng(nb + K)
    A = (rng.standard_normal((nb, K)) * (rng.random((nb, K)) < 0.3)).astype(np.float32)
    A[:, K // 2] = 0                                        # one all-zero coefficient column
    Href, cref = R.dict_stats(A)
    ws = ops.dict_workspace(16, 16, K, nb, "cuda")
    ws.view(torch.float32).fill_(float("nan"))
    H, c = ops.dict_stats(d(A), ws=ws)
    H, c = H.cpu().numpy(), float(c.cpu()[0])
    eh, ec = np.max(np.abs(H - Href)) / np.max(np.abs(Href)), abs(c - cref) / cref
    print(f"dict_stats ({nb}, {K}): H err {eh:.3e} of max|H|, c rel err {ec:.3e}")
    assert eh <= 1e-5
    assert ec <= 1e-6
    assert not H[K // 2].any() and not H[:, K // 2].any()


@pytest.mark.parametrize("shape", UPDATE_SHAPES)
def test_dict_update_one_iteration_vs_fp64(ops, shape):
    Dref, oref = update_case(shape)[4][1]
    D, obj, _ = run_update(ops, shape, 1)
    ed, eo = np.max(np.abs(D - Dref)) / np.max(np.abs(Dref)), np.max(np.abs(obj - oref) / oref)
    print(f"dict_update 1 it {shape}: D err {ed:.3e} of max|D|, obj rel err {eo:.3e}")
    assert np.isfinite(D).all() and np.isfinite(obj).all()
    assert ed <= 1e-5
    assert eo <= 1e-5
    K = shape[2]
    D0 = update_case(shape)[3]
    assert np.array_equal(D[:, K // 3], D0[:, K // 3])     # the atom no block uses is left as it is


@pytest.mark.parametrize("shape", UPDATE_SHAPES)
def test_dict_update_ten_iterations_vs_fp64(ops, shape):
    """Tolerance: four times the checker's float32-versus-fp64 deviation (recomputed here; recorded
    in DESIGN.md §8), no tighter than 1e-5.  Also test 4: obj never rises beyond the rounding slack."""
    n = shape[0]
    Yb, ob, A, D0, ref = update_case(shape)
    Dref, oref = ref[10]
    D32, o32 = R.dict_step(Yb[:, :n], ob[:, :n], A, D0, 10, dtype=np.float32)
    tol_d = max(1e-5, 4 * np.max(np.abs(D32 - Dref)) / np.max(np.abs(Dref)))
    tol_o = max(1e-5, 4 * np.max(np.abs(o32 - oref) / oref))
    assert np.all(o32[1:] <= o32[:-1] * (1 + 1e-6))          # the float32 checker stays inside the slack
    D, obj, _ = run_update(ops, shape, 10)
    ed, eo = np.max(np.abs(D - Dref)) / np.max(np.abs(Dref)), np.max(np.abs(obj - oref) / oref)
    print(f"dict_update 10 it {shape}: D err {ed:.3e} (tol {tol_d:.1e}), obj rel err {eo:.3e} (tol {tol_o:.1e}), "
          f"largest obj ratio {np.max(obj[1:] / obj[:-1]):.9f}")
    assert ed <= tol_d
    assert eo <= tol_o
    assert np.all(obj[1:] <= obj[:-1] * (1 + 1e-6))


@pytest.mark.parametrize("shape", UPDATE_SHAPES)
def test_dict_update_deterministic(ops, shape):
    D1, o1, c1 = run_update(ops, shape, 3)
    D2, o2, c2 = run_update(ops, shape, 3)
    assert np.array_equal(D1.view(np.uint32), D2.view(np.uint32))
    assert np.array_equal(o1.view(np.uint64), o2.view(np.uint64))
    assert c1 == c2


def test_zero_coefficients_leave_dictionary(ops):
    n, n_pad, K, nb = UPDATE_SHAPES[1]
    Yb, ob, A, D, _ = update_case(UPDATE_SHAPES[1])
    coefs, Dd = d(np.zeros_like(A)), d(D)
    _, c = ops.dict_stats(coefs)
    obj = ops.dict_update(d(Yb), d(ob), coefs, Dd, n, c, 2).cpu().numpy()
    assert float(c.cpu()[0]) == 0.0
    assert np.array_equal(Dd.cpu().numpy(), D)
    ref = 0.5 * np.sum((Yb[:, :n].astype(np.float64) * (ob[:, :n] != 0)) ** 2)
    assert np.all(np.abs(obj - ref) <= 1e-12 * ref)


def test_learn_dictionary_planted(ops):
    """rounds = 8, Nit = 50 on the planted problem (n = 64, K = 32, nb = 2,000).  The fp64 checker
    recovers 1 of the 32 planted atoms (3 %) in these 8 rounds (20 of 32 after 30), so the recovery
    bound here is 1 - 0.05 * 32 < 0 atoms: the objective bounds are the ones that bind."""
    from lrspnp.dictlearn import DictLearnConfig, learn_blocks, warm_start_supported
    Y, obs, Ds, D0 = R.planted_problem()
    cfg = DictLearnConfig(K=32, bb=8, lambda_ista=0.1, Nit=50, rounds=8, n_inner=10)
    assert warm_start_supported(64, 32, False)
    Dref, href, _ = R.learn(Y, obs, D0, 0.1, 50, 8, 10, warm=True)
    D, hist = learn_blocks(d(Y), d(obs), 64, d(D0), cfg)
    D, hist = D.cpu().numpy(), hist.cpu().numpy()
    gap = abs(hist[-1, -1] - href[-1, -1]) / href[-1, -1]
    rec, rec_ref = R.recovered(D, Ds), R.recovered(Dref, Ds)
    print(f"planted: objective {hist[0, 0]:.6g} -> {hist[-1, -1]:.6g} (fp64 checker {href[-1, -1]:.6g}, rel gap "
          f"{gap:.3e}); atoms recovered {rec} (checker {rec_ref}) of 32")
    assert hist.shape == (8, 11) and np.isfinite(hist).all()
    assert hist[-1, -1] < hist[0, 0]
    assert gap <= max(1e-4, 10 * 7.4e-9)
    assert rec >= rec_ref - 0.05 * 32
    assert np.allclose(np.linalg.norm(D.astype(np.float64), axis=0), 1.0, atol=1e-6)


def test_solver_learns_its_dictionary(ops):
    from lrspnp import DictLearnConfig, LrsPnP, LrsPnPConfig
    from lrspnp.data import mask_matrix, synthetic_cube, synthetic_dictionary, unfold
    cube, _, mask = synthetic_cube(24, 24, 40, seed=1)
    Y, M = unfold(cube), mask_matrix(mask, 40)
    dcfg = DictLearnConfig(K=64, Nit=20, rounds=2, n_inner=3)
    s = LrsPnP(Y, M, "learn", LrsPnPConfig(bb=8, sliding=8, Nit=20, dict_cfg=dcfg))
    assert tuple(s.D.shape) == (64, 64) and s.dict_history.shape == (2, 4)
    assert s.dict_history[-1, -1] < s.dict_history[0, 0]
    s.step()
    s.step()
    torch.cuda.synchronize()
    for t in (s.X, s.L1, s.L2, s.U, s.D):
        assert torch.isfinite(t).all()
    # an array D behaves as before: the new field and the "learn" branch leave that path alone
    D = synthetic_dictionary(64, 64, 0)
    a = LrsPnP(Y, M, D, LrsPnPConfig(bb=8, sliding=8, Nit=20, dict_cfg=dcfg))
    b = LrsPnP(Y, M, D, LrsPnPConfig(bb=8, sliding=8, Nit=20))
    for s2 in (a, b):
        s2.step()
        s2.step()
    torch.cuda.synchronize()
    for name in ("X", "L1", "L2", "U"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.dict_history is None


def test_refusals(ops):
    from lrspnp import _lib
    L = _lib.device_lib()
    n, n_pad, K, nb = UPDATE_SHAPES[1]
    Yb, ob, A, D, _ = update_case(UPDATE_SHAPES[1])
    Yd, od, Ad, Dd = d(Yb), d(ob), d(A), d(D)
    ws = ops.dict_workspace(n, n_pad, K, nb, "cuda")
    c = torch.ones(1, dtype=torch.float64, device="cuda")
    obj = torch.empty(2, dtype=torch.float64, device="cuda")
    H = torch.empty((K, K), dtype=torch.float32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert L.lrs_dict_update_f32(p(Yd), p(od), p(Ad), p(Dd), n, n_pad, 513, nb, p(c), 1, p(obj), p(ws), ws.numel(),
                                 None) == -2
    assert L.lrs_dict_stats_f32(p(Ad), nb, 513, p(H), p(c), p(ws), ws.numel(), None) == -2
    assert L.lrs_dict_update_f32(p(Yd), p(od), p(Ad), p(Dd), n, n_pad, K, nb, p(c), 1, p(obj), p(ws),
                                 ws.numel() - 1, None) == -3
    assert L.lrs_dict_update_f32(p(Yd), p(od), p(Ad), p(Dd), n, n_pad, K, nb, p(c), 1, None, p(ws), ws.numel(),
                                 None) == -1
    torch.cuda.synchronize()
    assert np.array_equal(Dd.cpu().numpy(), D)               # nothing was launched

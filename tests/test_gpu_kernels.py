"""Parity of the HIP kernels (through the C ABI) against the oracle, on a real MI355X.

Tolerances (written here, per kernel):
  * NLM prox kernel         : bit-exact vs the oracle's canonical closed form; <= 1 ulp vs skimage.
  * fused ISTA (coefs, Phi) : 1e-5 relative L2 per block vs the oracle (MFMA fp32 products sum in
                              a different order than the oracle's fp64-accumulated GEMVs).
  * alpha (||H||_2^2)       : 2 ulp of float32 vs numpy's float32 SVD; fro4 1e-6 relative.
  * SVT                     : 1e-5 relative L2 vs numpy float32 SVD (the reference's call).
  * ADMM update             : bit-exact vs the oracle (same float32 operation order).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lrspnp import ops as _ops
    return _ops


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _split(flat, sizes):
    out, o = [], 0
    for s in sizes:
        out.append(flat[o:o + s]); o += s
    return out


# ------------------------------------------------------------------------------------------ NLM
def test_nlm_kernel_bitexact_vs_oracle(ops):
    rng = np.random.default_rng(0)
    for K in (1, 5, 8, 17, 64, 256, 1296):
        for h in (1e-5, 4.9e-5, 3.2e-3, 0.05, 0.7):
            for scale in (1e-4, 1e-2, 1.0):
                g = (rng.standard_normal((7, K)) * scale).astype(np.float32)
                got = ops.nlm_col(torch.from_numpy(g).cuda(), h).cpu().numpy()
                for v in range(g.shape[0]):
                    ref = O.nlm_col(g[v], h)
                    assert np.array_equal(got[v].view(np.uint32), ref.view(np.uint32)), (K, h, scale, v)


def test_nlm_kernel_vs_skimage_golden(ops, golden):
    z = golden("nlm_golden.npz")
    tot = bad = 0
    for g, h, ref in zip(_split(z["col_in"], z["col_K"]), z["col_h"], _split(z["col_out"], z["col_K"])):
        got = ops.nlm_col(torch.from_numpy(g).cuda(), float(h)).cpu().numpy()
        d = np.abs(got.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
        assert d.max() <= 1
        tot += g.size; bad += int((d != 0).sum())
    assert bad <= max(1, tot // 10000)


def test_nlm_kernel_per_vector_h(ops):
    rng = np.random.default_rng(1)
    g = (rng.standard_normal((9, 256)) * 1e-3).astype(np.float32)
    hs = np.geomspace(1e-5, 1e-1, 9)
    got = ops.nlm_col(torch.from_numpy(g).cuda(), torch.from_numpy(hs).cuda()).cpu().numpy()
    for v in range(9):
        assert np.array_equal(got[v], O.nlm_col(g[v], hs[v]))


# ------------------------------------------------------------------------------------------ ISTA
def _rand_blocks(rng, nb, n, miss_frac, scale=0.3):
    Yb = (rng.standard_normal((nb, n)) * scale).astype(np.float32)
    obs = (rng.random((nb, n)) > miss_frac).astype(np.uint8)
    obs[0, :] = 1                                  # one fully observed block
    if nb > 2:
        obs[1, : n // 2] = 0                       # a heavily masked one
    Yb[obs == 0] = 0.0
    return Yb, obs


@pytest.mark.parametrize("bb,nb,Nit,variant,K", [
    (8, 300, 80, "spec2", 256), (8, 129, 100, "fro4", 256), (8, 64, 40, "soft", 256),
    (36, 20, 12, "fro4", 256), (36, 9, 10, "spec2", 256), (8, 70, 30, "matlab", 256), (36, 5, 8, "matlab", 256),
    (8, 70, 1, "matlab", 256), (36, 5, 1, "matlab", 256),
    # row-split kernel: dictionary sizes other than 256 (main_LRS_PnP.py:159-165 loads a trained
    # dictionary of unknown K), ragged n, many workgroups, every prox
    (36, 40, 10, "fro4", 128), (36, 17, 10, "fro4", 512), (36, 23, 8, "spec2", 200), (36, 30, 6, "soft", 256),
    (8, 50, 20, "fro4", 64), (8, 33, 20, "spec2", 100), (8, 20, 15, "soft", 300), (8, 21, 10, "fro4", 7),
    (20, 37, 10, "fro4", 256), (5, 19, 12, "spec2", 256), (36, 250, 5, "fro4", 256), (36, 3, 100, "fro4", 256),
    # K > 512: the generic dense-GEMM path (trained dictionaries of any size, main_LRS_PnP.py:159-165)
    (36, 21, 10, "fro4", 768), (36, 17, 8, "spec2", 1024), (8, 40, 12, "soft", 1024), (36, 9, 1, "matlab", 768),
    (8, 30, 15, "fro4", 600)])
def test_ista_kernel_vs_oracle(ops, bb, nb, Nit, variant, K):
    from lrspnp.data import synthetic_dictionary
    rng = np.random.default_rng(bb * 1000 + nb + K)
    n = bb * bb
    n_pad = -(-n // 16) * 16
    D = synthetic_dictionary(n, K, seed=3)
    Yb, obs = _rand_blocks(rng, nb, n, 0.2)
    alpha = np.empty(nb, np.float32); thr = np.empty(nb, np.float64)
    for j in range(nb):
        alpha[j], thr[j] = O.ista_alpha_h(D[obs[j].astype(bool)], 0.1, variant)
    prox = {"soft": O.PROX_SOFT, "matlab": O.PROX_NLM_MATLAB}.get(variant, O.PROX_NLM)
    Xo, PHIo = O.ista_batch(Yb, obs, D, alpha, thr, Nit, prox)
    pad = lambda a: np.pad(a, ((0, 0), (0, n_pad - n)))
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    phi, coefs = ops.ista(d(pad(Yb)), d(pad(obs)), d(D), n, d(alpha), d(thr), Nit, prox, want_coefs=True)
    phi = phi.cpu().numpy()[:, :n]
    coefs = coefs.cpu().numpy()
    worst = max(rel(coefs[j], Xo[j]) for j in range(nb))
    worst_phi = max(rel(phi[j], PHIo[j]) for j in range(nb))
    # The MATLAB variant's exp(-d/h^2) weights (no cutoff) amplify any ~1-ulp float32 difference:
    # d/h^2 ~ 1e2-1e3 at the reference's h, so the weights move by ~2 diff dg / h^2 ~ 1e-4 per
    # iteration.  The fused kernels hold one iteration from identical inputs to 1e-5 (the prox itself
    # is bit-exact, test_nlm_matlab_prox_bitexact); the generic path's GEMM rounds its gradient
    # differently, which the weights amplify even in one iteration.  So the bar is the oracle's own
    # sensitivity: the oracle re-run on inputs perturbed by 1 float32 ulp, and the kernel may differ
    # from the oracle by at most 4x that (and 1e-5).
    tol = 1e-5
    if variant == "matlab" and (Nit > 1 or K > 512):
        flip = np.where(rng.random(Yb.shape) < 0.5, -1.0, 1.0)
        Yp = (Yb.astype(np.float64) * (1.0 + flip * 2.0 ** -23)).astype(np.float32)
        Xp, PHIp = O.ista_batch(Yp, obs, D, alpha, thr, Nit, prox)
        sens = max(max(rel(Xp[j], Xo[j]) for j in range(nb)), max(rel(PHIp[j], PHIo[j]) for j in range(nb)))
        tol = max(1e-5, 4.0 * sens)
    assert worst < tol, (worst, tol)
    assert worst_phi < tol, (worst_phi, tol)


def _pattern_blocks(rng, nb, n, npat, miss_frac, scale=0.3):
    """Blocks that share `npat` observation patterns (ragged: one pattern holds > 16 blocks, one a
    single block); returns Yb, obs (per block), obs_pat, pat."""
    pats = (rng.random((npat, n)) > miss_frac).astype(np.uint8)
    pats[0, :] = 1
    if npat > 1:
        pats[1, : n // 2] = 0
    pat = rng.integers(0, npat, nb).astype(np.int32)
    pat[: min(nb, 18)] = 0
    if npat > 2:
        pat[pat == 2] = 3 % npat
        pat[-1] = 2
    obs = pats[pat]
    Yb = (rng.standard_normal((nb, n)) * scale).astype(np.float32)
    Yb[obs == 0] = 0.0
    return Yb, obs, pats, pat


def _pattern_case(ops, bb, nb, Nit, variant, K, npat, seed):
    from lrspnp.data import synthetic_dictionary
    rng = np.random.default_rng(seed)
    n = bb * bb
    n_pad = -(-n // 16) * 16
    D = synthetic_dictionary(n, K, seed=3)
    Yb, obs, pats, pat = _pattern_blocks(rng, nb, n, npat, 0.2)
    ap = np.empty(npat, np.float32); tp = np.empty(npat, np.float64)
    for k in range(npat):
        ap[k], tp[k] = O.ista_alpha_h(D[pats[k].astype(bool)], 0.1, variant)
    alpha, thr = ap[pat], tp[pat]
    prox = {"soft": O.PROX_SOFT, "matlab": O.PROX_NLM_MATLAB}.get(variant, O.PROX_NLM)
    pad = lambda a: np.pad(a, ((0, 0), (0, n_pad - n)))
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    plan, nt = ops.ista_pat_plan(pat, npat)
    ws = ops.ista_pat_prepare(d(D), d(pad(pats)), n)
    args = dict(Yb=d(pad(Yb)), obs_pat=d(pad(pats)), plan=d(plan), ntiles=nt, K=K, n=n, alpha=d(alpha),
                thr=d(thr), Nit=Nit, ws=ws, prox=prox)
    return rng, n, D, Yb, obs, alpha, thr, prox, args, d, pad


@pytest.mark.parametrize("bb,nb,Nit,variant,K,npat", [
    (36, 40, 12, "fro4", 256, 3), (36, 37, 10, "spec2", 256, 5), (36, 21, 8, "soft", 256, 2),
    (36, 19, 6, "matlab", 256, 4), (36, 35, 10, "fro4", 128, 3), (36, 18, 8, "fro4", 512, 2),
    (36, 23, 10, "fro4", 200, 4), (20, 50, 10, "fro4", 256, 6), (8, 40, 10, "fro4", 7, 3),
    (8, 33, 12, "spec2", 64, 2), (36, 3, 100, "fro4", 256, 1), (36, 70, 1, "fro4", 256, 3)])
def test_ista_pattern_gram_vs_oracle(ops, bb, nb, Nit, variant, K, npat):
    """The per-pattern Gram path (lrs_ista_pat_f32: g = x + (b - Q_p x) / alpha) against the oracle's
    per-block ista() at 1e-5 (the MATLAB prox: its own sensitivity bar, as above), and against the
    row-split kernel on the same blocks at 1e-5."""
    rng, n, D, Yb, obs, alpha, thr, prox, args, d, pad = _pattern_case(ops, bb, nb, Nit, variant, K, npat,
                                                                        bb * 7 + nb + K + npat)
    Xo, PHIo = O.ista_batch(Yb, obs, D, alpha, thr, Nit, prox)
    phi, coefs = ops.ista_pat(**args, want_coefs=True)
    assert np.all(phi.cpu().numpy()[:, n:] == 0)
    phi = phi.cpu().numpy()[:, :n]
    coefs = coefs.cpu().numpy()
    tol = 1e-5
    if variant == "matlab" and Nit > 1:
        flip = np.where(rng.random(Yb.shape) < 0.5, -1.0, 1.0)
        Yp = (Yb.astype(np.float64) * (1.0 + flip * 2.0 ** -23)).astype(np.float32)
        Xp, PHIp = O.ista_batch(Yp, obs, D, alpha, thr, Nit, prox)
        sens = max(max(rel(Xp[j], Xo[j]) for j in range(nb)), max(rel(PHIp[j], PHIo[j]) for j in range(nb)))
        tol = max(1e-5, 4.0 * sens)
    assert max(rel(coefs[j], Xo[j]) for j in range(nb)) < tol
    assert max(rel(phi[j], PHIo[j]) for j in range(nb)) < tol
    phr, cor = ops.ista(args["Yb"], d(pad(obs)), d(D), n, args["alpha"], args["thr"], Nit, prox, want_coefs=True)
    assert max(rel(coefs[j], cor.cpu().numpy()[j]) for j in range(nb)) < max(tol, 1e-5)


def test_ista_pattern_gram_grid_and_warm_start_bitwise(ops):
    """lrs_ista_pat_f32's bounded grid (max_workgroups) and warm-start slices give the one-launch
    result bit for bit; repeated calls are deterministic."""
    _, n, D, Yb, obs, alpha, thr, prox, args, d, pad = _pattern_case(ops, 36, 16 * 5 + 7, 12, "fro4", 256, 4, 91)
    phi0, c0 = ops.ista_pat(**args, want_coefs=True)
    phi1, c1 = ops.ista_pat(**args, want_coefs=True, max_workgroups=2)
    assert torch.equal(phi0, phi1) and torch.equal(c0, c1)
    phi2, c2 = ops.ista_pat(**args, want_coefs=True)
    assert torch.equal(phi0, phi2) and torch.equal(c0, c2)
    a = dict(args)
    co = torch.zeros_like(c0)
    done = 0
    for k, it in enumerate((5, 4, 3)):
        a["Nit"] = it
        ph, _ = ops.ista_pat(**a, coefs=co, want_coefs=True, warm_start=k > 0)
        done += it
    assert done == 12 and torch.equal(co, c0) and torch.equal(ph, phi0)


@pytest.mark.parametrize("bb,nb,Nit,variant,K", [(36, 23, 10, "fro4", 256), (8, 70, 20, "spec2", 256),
                                                  (36, 12, 6, "soft", 100), (20, 19, 9, "fro4", 512)])
def test_ista_generic_path_vs_oracle(ops, bb, nb, Nit, variant, K):
    """lrs_ista_opts.algorithm = LRS_ISTA_ALGO_GENERIC (the path K > 512 takes) at sizes the fused
    kernels also serve: 1e-5 vs the oracle, and 1e-5 vs the fused kernels."""
    from lrspnp.data import synthetic_dictionary
    rng = np.random.default_rng(bb * 31 + nb + K)
    n = bb * bb
    n_pad = -(-n // 16) * 16
    D = synthetic_dictionary(n, K, seed=5)
    Yb, obs = _rand_blocks(rng, nb, n, 0.2)
    alpha = np.empty(nb, np.float32); thr = np.empty(nb, np.float64)
    for j in range(nb):
        alpha[j], thr[j] = O.ista_alpha_h(D[obs[j].astype(bool)], 0.1, variant)
    prox = {"soft": O.PROX_SOFT}.get(variant, O.PROX_NLM)
    Xo, PHIo = O.ista_batch(Yb, obs, D, alpha, thr, Nit, prox)
    pad = lambda a: np.pad(a, ((0, 0), (0, n_pad - n)))
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    res = {}
    for algo in (0, 1):
        phi, coefs = ops.ista(d(pad(Yb)), d(pad(obs)), d(D), n, d(alpha), d(thr), Nit, prox, want_coefs=True,
                              algorithm=algo)
        res[algo] = (phi.cpu().numpy()[:, :n], coefs.cpu().numpy())
        assert np.all(phi.cpu().numpy()[:, n:] == 0)
    phi, coefs = res[1]
    assert max(rel(coefs[j], Xo[j]) for j in range(nb)) < 1e-5
    assert max(rel(phi[j], PHIo[j]) for j in range(nb)) < 1e-5
    assert max(rel(coefs[j], res[0][1][j]) for j in range(nb)) < 1e-5


def test_ista_bounded_grid_is_bitwise_the_same(ops):
    """lrs_ista_opts.max_workgroups (the row-split kernel persistent over 16-block tiles, as the DIP
    mains run it beside the training): the same result bit for bit, ragged last tile included."""
    from lrspnp.data import synthetic_dictionary
    rng = np.random.default_rng(77)
    n, nb, K = 36 * 36, 16 * 9 + 5, 256
    D = synthetic_dictionary(n, K, seed=3)
    Yb, obs = _rand_blocks(rng, nb, n, 0.2)
    alpha = np.empty(nb, np.float32); thr = np.empty(nb, np.float64)
    for j in range(nb):
        alpha[j], thr[j] = O.ista_alpha_h(D[obs[j].astype(bool)], 0.1, "fro4")
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = []
    for mw in (0, 1, 3, 7, 1000):
        phi, coefs = ops.ista(d(Yb), d(obs), d(D), n, d(alpha), d(thr), 12, ops.PROX_NLM, want_coefs=True,
                              max_workgroups=mw)
        torch.cuda.synchronize()
        out.append((phi.cpu().numpy(), coefs.cpu().numpy()))
    for o in out[1:]:
        assert np.array_equal(o[0], out[0][0]) and np.array_equal(o[1], out[0][1])
    Xo, PHIo = O.ista_batch(Yb, obs, D, alpha, thr, 12, O.PROX_NLM)
    assert max(rel(out[0][1][j], Xo[j]) for j in range(nb)) < 1e-5


@pytest.mark.parametrize("K,prox", [(256, "nlm"), (100, "nlm"), (512, "soft"), (256, "matlab")])
def test_ista_warm_start_slices_are_one_launch(ops, K, prox):
    """lrs_ista_opts.warm_start (the time-sliced sparse coding beside the DIP, LrsPnPConfig.
    ista_slices_dip): Nit iterations split over several launches that continue from the coefficients
    give the one-launch Phi and coefficients bit for bit; unsupported (no coefs) is refused."""
    from lrspnp.data import synthetic_dictionary
    from lrspnp._lib import LrsError
    rng = np.random.default_rng(5)
    n, nb = 36 * 36, 16 * 3 + 7
    pr = {"nlm": ops.PROX_NLM, "soft": ops.PROX_SOFT, "matlab": ops.PROX_NLM_MATLAB}[prox]
    D = synthetic_dictionary(n, K, seed=4)
    Yb, obs = _rand_blocks(rng, nb, n, 0.2)
    alpha = np.empty(nb, np.float32); thr = np.empty(nb, np.float64)
    for j in range(nb):
        alpha[j], thr[j] = O.ista_alpha_h(D[obs[j].astype(bool)], 0.1, "soft" if prox == "soft" else "fro4")
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    args = (d(Yb), d(obs), d(D), n, d(alpha), d(thr))
    phi1, co1 = ops.ista(*args, 13, pr, want_coefs=True)
    co = torch.full((nb, K), float("nan"), device="cuda")
    done = 0
    for k, it in enumerate((4, 1, 5, 3)):
        phi, _ = ops.ista(*args, it, pr, coefs=co, want_coefs=True, warm_start=k > 0)
        done += it
    torch.cuda.synchronize()
    assert done == 13
    assert torch.equal(phi, phi1) and torch.equal(co, co1)
    with pytest.raises(LrsError):
        ops.ista(*args, 2, pr, warm_start=True)
    # warm start exists only on the row-split kernel: the generic dense-GEMM path (algorithm 1, or
    # K > 512) refuses it instead of silently restarting from zero
    with pytest.raises(LrsError):
        ops.ista(*args, 2, pr, coefs=co, want_coefs=True, warm_start=True, algorithm=1)


def test_ista_warm_start_refused_above_k512(ops):
    from lrspnp.data import synthetic_dictionary
    from lrspnp._lib import LrsError
    rng = np.random.default_rng(6)
    n, nb, K = 8 * 8, 20, 768
    D = synthetic_dictionary(n, K, seed=4)
    Yb, obs = _rand_blocks(rng, nb, n, 0.2)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    co = torch.zeros((nb, K), device="cuda")
    with pytest.raises(LrsError):
        ops.ista(d(Yb), d(obs), d(D), n, d(np.ones(nb, np.float32)), d(np.full(nb, 0.05)), 2, ops.PROX_NLM,
                 coefs=co, want_coefs=True, warm_start=True)


def test_nlm_col_top_of_k_range(ops):
    """k_nlm_col at the documented top of its range, K = 16384: (K + 10) floats of LDS exceed
    64 KiB and the launch is opted into more; bit-exact vs the oracle like every other K."""
    g = np.random.default_rng(3).uniform(0, 1, (2, 16384)).astype(np.float32)
    out = ops.nlm_col(torch.from_numpy(g).cuda(), 0.04).cpu().numpy()
    for v in range(2):
        np.testing.assert_array_equal(out[v], O.nlm_col(g[v], 0.04))


def test_ista_kernel_vs_reference_golden(ops, golden):
    """Reference `ista` outputs (captured from the unmodified reference, gen_golden.py)."""
    from lrspnp.data import synthetic_dictionary
    z = golden("ista_golden.npz")
    D = synthetic_dictionary(1296, 256, 0)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for variant in ("spec2", "fro4"):
        Y, obs = z[variant + "_y"], z[variant + "_obs"]
        nb = Y.shape[0]
        alpha = np.empty(nb, np.float32); thr = np.empty(nb, np.float64)
        for j in range(nb):
            alpha[j], thr[j] = O.ista_alpha_h(D[obs[j].astype(bool)], 0.1, variant)
        phi, coefs = ops.ista(d(Y), d(obs), d(D), 1296, d(alpha), d(thr), int(z[variant + "_Nit"]), 0,
                              want_coefs=True)
        for j in range(nb):
            assert rel(coefs.cpu().numpy()[j], z[variant + "_coefs"][j]) < 1e-5
            assert rel(phi.cpu().numpy()[j], z[variant + "_phi"][j]) < 1e-5


def test_ista_deterministic(ops):
    from lrspnp.data import synthetic_dictionary
    rng = np.random.default_rng(5)
    D = synthetic_dictionary(64, 256, 0)
    Yb, obs = _rand_blocks(rng, 1000, 64, 0.1)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    alpha = d(np.full(1000, 5.0, np.float32)); thr = d(np.full(1000, 1e-3))
    a = ops.ista(d(Yb), d(obs), d(D), 64, alpha, thr, 20, 0)
    b = ops.ista(d(Yb), d(obs), d(D), 64, alpha, thr, 20, 0)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------ alpha
@pytest.mark.parametrize("n,variant", [(64, "spec2"), (64, "fro4"), (64, "soft"), (1296, "spec2"),
                                       (1296, "fro4")])
def test_alpha_kernel_vs_numpy(ops, n, variant):
    from lrspnp.data import synthetic_dictionary
    rng = np.random.default_rng(n)
    D = synthetic_dictionary(n, 256, 0)
    n_pad = -(-n // 16) * 16
    npat = 6
    obs = (rng.random((npat, n)) > np.linspace(0.0, 0.8, npat)[:, None]).astype(np.uint8)
    obs[0] = 1
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    mode = {"spec2": 0, "fro4": 1, "soft": 2}[variant]
    a, t = ops.ista_alpha(d(D), d(np.pad(obs, ((0, 0), (0, n_pad - n)))), n, mode, 0.1)
    a = a.cpu().numpy(); t = t.cpu().numpy()
    for j in range(npat):
        ra, rt = O.ista_alpha_h(D[obs[j].astype(bool)], 0.1, variant)
        if variant == "fro4":
            assert abs(a[j] - ra) <= 1e-6 * ra
        else:
            assert abs(int(a[j].view(np.int32)) - int(np.float32(ra).view(np.int32))) <= 2, (j, a[j], ra)
        assert abs(t[j] - rt) <= 4e-7 * rt


# ------------------------------------------------------------------------------------------ SVT
@pytest.mark.parametrize("method", ["tri", "jacobi"])
@pytest.mark.parametrize("P,B,rank,noise", [(1296, 128, 8, 0.12), (4000, 198, 8, 0.02), (500, 60, 3, 0.002),
                                            (777, 45, 5, 0.05),
                                            # above 198 bands the packed triangle lives in the workspace
                                            # (the 224-band cubes of configs[3]/[4]); 256 is the limit
                                            (3000, 199, 8, 0.02), (3000, 200, 8, 0.02), (5000, 224, 8, 0.02),
                                            (4096, 256, 8, 0.02)])
def test_svt_kernel_vs_numpy(ops, P, B, rank, noise, method):
    _svt_vs_numpy(ops, P, B, rank, noise, method)


@pytest.mark.parametrize("method", ["tri", "jacobi"])
@pytest.mark.parametrize("P,B", [(400, 201), (400, 208), (400, 209)])
def test_svt_shape_class_boundaries(ops, P, B, method):
    """Both sides of the boundaries between the B <= 256 shape classes (csrc/svt_ws.h): 201 is the first
    band count of the <16, 64> apply, 208 the last of the <13, 4> Gram, 209 the first of the <16, 8>
    Gram.  The checks of test_svt_kernel_vs_numpy; the tridiagonal path also over several workgroups,
    bit for bit."""
    _svt_vs_numpy(ops, P, B, 8, 0.02, method, multi_wg_too=(method == "tri"))


def _svt_vs_numpy(ops, P, B, rank, noise, method, multi_wg_too=False):
    rng = np.random.default_rng(P + B)
    Z = (rng.random((P, rank)) @ rng.random((rank, B)) * 0.3 + noise * rng.standard_normal((P, B)))
    X = Z.astype(np.float32)
    L2 = (0.01 * rng.standard_normal((P, B))).astype(np.float32)
    c2 = np.float32(1 / 0.9)
    tau = float(np.float32(1 / 0.9))
    ref = O.svt(X + c2 * L2, 1 / 0.9)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ws = ops.svt_workspace(P, B, "cuda")
    s = torch.empty(B, dtype=torch.float64, device="cuda")
    U = ops.svt(d(X), d(L2), c2, tau, ws, s_out=s, warm=False, method=method).cpu().numpy()
    assert rel(U, ref) < 1e-5
    sref = np.linalg.svd((X + c2 * L2).astype(np.float64), compute_uv=False)
    assert rel(s.cpu().numpy(), sref) < 1e-9
    path = ops.svt_state(ws, P, B)[4]
    assert path == (1 if method == "tri" else 3), path     # the tridiagonal path certified itself
    if multi_wg_too:
        wsm = ops.svt_workspace(P, B, "cuda")
        sm = torch.empty(B, dtype=torch.float64, device="cuda")
        Um = ops.svt(d(X), d(L2), c2, tau, wsm, s_out=sm, warm=False, method=method, multi_wg=True).cpu().numpy()
        assert ops.svt_state(wsm, P, B)[4] == path
        assert np.array_equal(Um.view(np.uint32), U.view(np.uint32))
        assert np.array_equal(sm.cpu().numpy(), s.cpu().numpy())
    # warm start from the previous eigenvectors on a perturbed matrix
    X2 = (X + 1e-3 * rng.standard_normal((P, B))).astype(np.float32)
    U2 = ops.svt(d(X2), d(L2), c2, tau, ws, warm=True, method=method).cpu().numpy()
    assert rel(U2, O.svt(X2 + c2 * L2, 1 / 0.9)) < 1e-5


@pytest.mark.parametrize("B", [64, 197, 224])
@pytest.mark.parametrize("exact", [True, False])
def test_svt_repeated_singular_values(ops, B, exact):
    """Repeated singular values.  exact: Z = 2 [I; 0] plus a rank-3 term on rows the identity does
    not touch, so the Gram has the eigenvalue 4 exactly B - 3 times and T splits into identical
    blocks: inverse iteration returns non-orthogonal vectors, the certificate fails and the
    workgroup falls back to Jacobi.  Otherwise (float32-rounded orthonormal columns, a tight
    cluster) the Newton-Schulz repair keeps the tridiagonal path.  U matches LAPACK either way."""
    rng = np.random.default_rng(B)
    P = 3 * B
    if exact:
        X = np.zeros((P, B), np.float32)
        X[:B, :B] = 2.0 * np.eye(B, dtype=np.float32)
        X[B:, :3] = (0.5 * rng.standard_normal((P - B, 3))).astype(np.float32)
    else:
        Q, _ = np.linalg.qr(rng.standard_normal((P, B)))
        X = (2.0 * Q).astype(np.float32)
        X[:, :3] += (0.5 * rng.standard_normal((P, 3))).astype(np.float32)
    ref = O.svt(X, 1 / 0.9)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ws = ops.svt_workspace(P, B, "cuda")
    U = ops.svt(d(X), None, 1.0, float(np.float32(1 / 0.9)), ws).cpu().numpy()
    assert rel(U, ref) < 1e-5
    path = ops.svt_state(ws, P, B)[4]
    assert path == (2 if exact else 1), path
    # the multi-workgroup chain takes the same path and gives the same U bit for bit
    Um = ops.svt(d(X), None, 1.0, float(np.float32(1 / 0.9)), ws, multi_wg=True).cpu().numpy()
    assert ops.svt_state(ws, P, B)[4] == path and np.array_equal(Um.view(np.uint32), U.view(np.uint32))


@pytest.mark.parametrize("P,B", [(1296, 128), (4000, 198), (500, 60), (777, 45), (300, 7), (2000, 197),
                                 (3000, 224), (3000, 255)])
def test_svt_multi_workgroup_bit_identical(ops, P, B):
    """LRS_SVT_MULTI_WG (the eigenvalue, inverse-iteration and back-transformation phases over many
    workgroups, for a row-slab shard whose eigensolver is on the critical path): U and the singular
    values bit-identical to the one-workgroup chain, on the tridiagonal path."""
    rng = np.random.default_rng(3 * P + B)
    Z = (rng.random((P, 6)) @ rng.random((6, B)) * 0.3 + 0.05 * rng.standard_normal((P, B)))
    X = Z.astype(np.float32)
    L2 = (0.01 * rng.standard_normal((P, B))).astype(np.float32)
    c2 = np.float32(1 / 0.9)
    tau = float(np.float32(1 / 0.9))
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = {}
    for mw in (False, True):
        ws = ops.svt_workspace(P, B, "cuda")
        s = torch.empty(B, dtype=torch.float64, device="cuda")
        U = ops.svt(d(X), d(L2), c2, tau, ws, s_out=s, multi_wg=mw).cpu().numpy()
        out[mw] = (U, s.cpu().numpy(), ops.svt_state(ws, P, B)[4])
    assert out[True][2] == out[False][2] == 1
    assert np.array_equal(out[True][0].view(np.uint32), out[False][0].view(np.uint32))
    assert np.array_equal(out[True][1], out[False][1])
    assert rel(out[True][0], O.svt(X + c2 * L2, 1 / 0.9)) < 1e-5


# ------------------------------------------------------------------------------------------ ADMM
def test_admm_update_bitexact_vs_oracle(ops):
    rng = np.random.default_rng(11)
    for (P, B, bb) in [(1296, 128, 36), (400, 30, 8), (103, 29, 7)]:
        rows, cols = O.block_grid(P, B, bb, bb)
        nb = rows.size
        n = bb * bb
        n_pad = -(-n // 16) * 16
        mk = lambda *s: rng.standard_normal(s).astype(np.float32)
        Y, U, L1, L2, X = mk(P, B), mk(P, B), mk(P, B), mk(P, B), mk(P, B)
        M = (rng.random((P, B)) > 0.1).astype(np.float32)
        PHI = mk(nb, n)
        Xo, L1o, L2o, IMo = (np.empty_like(X) for _ in range(4))
        import ctypes
        O.lib().oracle_admm_update(P, B, bb, nb, rows, cols, PHI, Y, M, U, L1, L2, 0.5, np.float32(0.15),
                                   np.float32(0.9), Xo, L1o, L2o, IMo.ctypes.data_as(ctypes.c_void_p), None)
        from lrspnp import ops as lops
        r, c = lops.block_grid(P, B, bb, bb)
        rs, cs = np.unique(r), np.unique(c)
        rlo, rhi = lops.cover_ranges(P, bb, rs)
        clo, chi = lops.cover_ranges(B, bb, cs)
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        grid = dict(rstarts=d(rs), cstarts=d(cs), nbr=rs.size, rlo=d(rlo), rhi=d(rhi), clo=d(clo), chi=d(chi))
        Xd, L1d, L2d = d(X), d(L1), d(L2)
        im = torch.empty_like(Xd)
        norms = torch.zeros(3, dtype=torch.float64, device="cuda")
        lops.admm_update(Xd, L1d, L2d, d(Y), d(M), d(U), d(np.pad(PHI, ((0, 0), (0, n_pad - n)))), bb, grid,
                         np.float32(0.5), np.float32(0.15), np.float32(0.9), norms=norms, imout=im)
        assert np.array_equal(im.cpu().numpy(), IMo)
        assert np.array_equal(Xd.cpu().numpy(), Xo)
        assert np.array_equal(L1d.cpu().numpy(), L1o)
        assert np.array_equal(L2d.cpu().numpy(), L2o)
        nref = [np.sum((Xo.astype(np.float64) - X) ** 2), np.sum((L1o.astype(np.float64) - L1) ** 2),
                np.sum((L2o.astype(np.float64) - L2) ** 2)]
        assert np.allclose(norms.cpu().numpy(), nref, rtol=1e-10)


def _admm_case(ops, P, B, bb, sliding, seed, want_norms=True, want_imout=True):
    """One lrs_admm_update_f32 call on the grid (P, B, bb, sliding) next to oracle_admm_update on the
    same corner list.  Returns the kernel's (X, L1, L2, imout, norms), the oracle's (X, L1, L2, imout)
    and the inputs (X, L1, L2)."""
    import ctypes
    rng = np.random.default_rng(seed)
    rows, cols = O.block_grid(P, B, bb, sliding)
    nb, n = rows.size, bb * bb
    n_pad = -(-n // 16) * 16
    mk = lambda *s: rng.standard_normal(s).astype(np.float32)
    Y, U, L1, L2, X = mk(P, B), mk(P, B), mk(P, B), mk(P, B), mk(P, B)
    M = (rng.random((P, B)) > 0.1).astype(np.float32)
    PHI = mk(nb, n)
    Xo, L1o, L2o, IMo = (np.empty_like(X) for _ in range(4))
    O.lib().oracle_admm_update(P, B, bb, nb, rows, cols, PHI, Y, M, U, L1, L2, 0.5, np.float32(0.15),
                               np.float32(0.9), Xo, L1o, L2o, IMo.ctypes.data_as(ctypes.c_void_p), None)
    r, c = ops.block_grid(P, B, bb, sliding)
    assert np.array_equal(r, rows) and np.array_equal(c, cols)
    rs, cs = np.unique(r), np.unique(c)
    rlo, rhi = ops.cover_ranges(P, bb, rs)
    clo, chi = ops.cover_ranges(B, bb, cs)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    grid = dict(rstarts=d(rs), cstarts=d(cs), nbr=rs.size, rlo=d(rlo), rhi=d(rhi), clo=d(clo), chi=d(chi))
    Xd, L1d, L2d = d(X), d(L1), d(L2)
    im = torch.full_like(Xd, 7.0) if want_imout else None
    norms = torch.full((3,), 7.0, dtype=torch.float64, device="cuda") if want_norms else None
    ops.admm_update(Xd, L1d, L2d, d(Y), d(M), d(U), d(np.pad(PHI, ((0, 0), (0, n_pad - n)))), bb, grid,
                    np.float32(0.5), np.float32(0.15), np.float32(0.9), norms=norms, imout=im)
    got = (Xd.cpu().numpy(), L1d.cpu().numpy(), L2d.cpu().numpy(), im.cpu().numpy() if want_imout else None,
           norms.cpu().numpy() if want_norms else None)
    return got, (Xo, L1o, L2o, IMo), (X, L1, L2)


def _admm_check(got, ref, inp):
    bits = lambda a: a.view(np.uint32)
    for g, r in zip(got[:3], ref[:3]):
        assert np.array_equal(bits(g), bits(r))
    if got[3] is not None:
        assert np.array_equal(bits(got[3]), bits(ref[3]))
    if got[4] is not None:
        # the atomics leave the order of the fp64 sums free: not bit-exact
        nref = [np.sum((r.astype(np.float64) - x) ** 2) for r, x in zip(ref[:3], inp)]
        assert np.allclose(got[4], nref, rtol=1e-10, atol=0.0)


@pytest.mark.parametrize("P,B,bb,sliding", [(40, 33, 8, 3), (20 * 20, 24, 8, 4), (50, 50, 8, 1),
                                            (1100, 500, 36, 36)])
def test_admm_update_overlapping_covers_bitexact(ops, P, B, bb, sliding):
    """The gather over overlapping covers (sliding < bb: up to bb^2 blocks per element, walked in the
    reference's block order), and P * B = 550000 > 2048 * 256 threads, where every thread takes a second
    element of the grid-stride loop."""
    _admm_check(*_admm_case(ops, P, B, bb, sliding, seed=P + sliding))


@pytest.mark.parametrize("want_norms,want_imout", [(False, True), (True, False), (False, False)])
def test_admm_update_optional_outputs(ops, want_norms, want_imout):
    """norms = NULL and imout = NULL: X, L1 and L2 keep the bits of the full call."""
    full = _admm_case(ops, 40, 33, 8, 3, seed=21)
    part = _admm_case(ops, 40, 33, 8, 3, seed=21, want_norms=want_norms, want_imout=want_imout)
    _admm_check(*full)
    _admm_check(*part)
    for a, b in zip(full[0][:3], part[0][:3]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_cover_ranges_refusal_and_gap(ops):
    from lrspnp._lib import LrsError
    for starts in ([0, 4, 4, 8], [0, 8, 4]):
        with pytest.raises(LrsError, match="LRS_E_INVALID"):
            ops.cover_ranges(12, 4, np.array(starts, np.int32))
    lo, hi = ops.cover_ranges(14, 4, np.array([0, 10], np.int32))       # nothing covers 4..9
    covered = np.array([x < 4 or x >= 10 for x in range(14)])
    assert np.all(hi[~covered] < lo[~covered])
    assert np.all(lo[:4] == 0) and np.all(hi[:4] == 0) and np.all(lo[10:] == 1) and np.all(hi[10:] == 1)


def _im2col_case(ops, P, B, bb, sliding, n_pad, with_L, seed):
    rng = np.random.default_rng(seed)
    mu = np.float32(0.15)
    X = rng.standard_normal((P, B)).astype(np.float32)
    Lm = rng.standard_normal((P, B)).astype(np.float32) if with_L else None
    # an element that cancels to 0 (X + L/mu = 1 - mu/mu), a -0.0 and a +0.0: all unobserved.  (0, 0) and
    # (1, 2) lie in the first block of every grid; with sliding < bb the last rows may be in no block
    X[0, 0] = 1.0
    X[1, 2] = -0.0
    X[P // 2, B // 2] = 0.0
    if with_L:
        Lm[0, 0] = -mu
        Lm[1, 2] = -0.0
        Lm[P // 2, B // 2] = 0.0
    else:
        X[0, 0] = 0.0
    Z = X + Lm / mu if with_L else X
    assert Z.dtype == np.float32 and Z[0, 0] == 0.0 and np.signbit(Z[1, 2])
    rows, cols = O.block_grid(P, B, bb, sliding)
    ref = O.im2col(Z, bb, rows, cols)
    r, c = ops.block_grid(P, B, bb, sliding)
    assert np.array_equal(r, rows) and np.array_equal(c, cols)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    nb, n = rows.size, bb * bb
    Yb = torch.full((nb, n_pad), 7.0, dtype=torch.float32, device="cuda")        # the padding must be written
    obs = torch.full((nb, n_pad), 255, dtype=torch.uint8, device="cuda")
    ops.im2col(d(X), d(Lm) if with_L else None, mu, bb, d(r), d(c), n_pad, Yb=Yb, obs=obs, want_obs=True)
    Yb, obs = Yb.cpu().numpy(), obs.cpu().numpy()
    assert np.array_equal(Yb[:, :n].view(np.uint32), ref.view(np.uint32))
    assert not Yb[:, n:].view(np.uint32).any()                                   # exactly +0.0
    assert np.array_equal(obs[:, :n], (ref != 0).astype(np.uint8))
    assert not obs[:, n:].any()
    assert (ref == 0).sum() >= 3 and np.signbit(ref[ref == 0]).any()
    Yb2 = ops.im2col(d(X), d(Lm) if with_L else None, mu, bb, d(r), d(c), n_pad).cpu().numpy()   # obs = NULL
    assert np.array_equal(Yb2.view(np.uint32), Yb.view(np.uint32))


@pytest.mark.parametrize("with_L", [True, False])
@pytest.mark.parametrize("extra_pad", [0, 16])
@pytest.mark.parametrize("P,B,bb,sliding", [(103, 29, 7, 7), (40, 33, 8, 3), (9, 9, 9, 1)])
def test_im2col_bitexact_vs_oracle(ops, P, B, bb, sliding, extra_pad, with_L):
    """lrs_im2col_f32 alone: block vectors of X + L/mu in float32, bit for bit; the padding columns
    exactly 0; obs 1 exactly where the value is non-zero."""
    n_pad = -(-bb * bb // 16) * 16 + extra_pad
    _im2col_case(ops, P, B, bb, sliding, n_pad, with_L, seed=P)


def test_im2col_grid_stride_wrap(ops):
    """nb * n_pad = 249001 * 80 > 65536 * 256: the grid-stride loop's second trip."""
    assert O.block_grid(1500, 1500, 8, 3)[0].size * 80 > 65536 * 256
    _im2col_case(ops, 1500, 1500, 8, 3, 80, True, seed=1500)


def test_ista_both_product_precisions_match_oracle():
    """The resident kernel's products in exact f32 MFMA and in split-bf16 MFMA (the default):
    both within 1e-5 of the oracle, and within 1e-6 of each other."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lrspnp import _lib, ops
    from lrspnp.data import synthetic_dictionary
    L = _lib.device_lib()
    rng = np.random.default_rng(11)
    nb, n = 300, 64
    D = synthetic_dictionary(n, 256, 0)
    Yb = (rng.standard_normal((nb, n)) * 0.3).astype(np.float32)
    obs = (rng.random((nb, n)) > 0.1).astype(np.uint8)
    Yb[obs == 0] = 0
    Dd, Yd, od = (torch.from_numpy(a).cuda() for a in (D, Yb, obs))
    alpha, thr = ops.ista_alpha(Dd, od, n, ops.ALPHA_SPEC2, 0.1)
    al, th = alpha.cpu().numpy(), thr.cpu().numpy()
    coefs_o, phi_o = O.ista_batch(Yb, obs, D, al, th, 30)
    out = {}
    for prec in (0, 1, None):          # lrs_ista_opts.precision per call (None: default = split-bf16)
        phi, coefs = ops.ista(Yd, od, Dd, n, alpha, thr, 30, ops.PROX_NLM, want_coefs=True, precision=prec)
        torch.cuda.synchronize()
        out[prec] = (phi.cpu().numpy()[:, :n], coefs.cpu().numpy())
        assert rel(out[prec][0], phi_o) < 1e-5 and rel(out[prec][1], coefs_o) < 1e-5
    assert rel(out[1][0], out[0][0]) < 1e-6
    assert np.array_equal(out[None][0], out[1][0])      # no process-wide mode: the default is per call


def test_ista_soft_both_product_precisions_match_oracle():
    """The resident kernels with the soft prox: k_ista_res<256, true> (exact f32 products) and
    k_ista_b3 (split-bf16), both within 1e-5 of the oracle and within 1e-6 of each other.  nb = 130
    gives the 128-block workgroups of k_ista_res a second, ragged one and the 64-block workgroups of
    the split kernels a third."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lrspnp import ops
    from lrspnp.data import synthetic_dictionary
    rng = np.random.default_rng(12)
    nb, n = 130, 64
    D = synthetic_dictionary(n, 256, 0)
    Yb = (rng.standard_normal((nb, n)) * 0.3).astype(np.float32)
    obs = (rng.random((nb, n)) > 0.1).astype(np.uint8)
    Yb[obs == 0] = 0
    Dd, Yd, od = (torch.from_numpy(a).cuda() for a in (D, Yb, obs))
    alpha, thr = ops.ista_alpha(Dd, od, n, ops.ALPHA_SOFT, 0.1)
    al, th = alpha.cpu().numpy(), thr.cpu().numpy()
    coefs_o, phi_o = O.ista_batch(Yb, obs, D, al, th, 10, O.PROX_SOFT)
    out = {}
    for prec in (0, 1):
        phi, coefs = ops.ista(Yd, od, Dd, n, alpha, thr, 10, ops.PROX_SOFT, want_coefs=True, precision=prec)
        torch.cuda.synchronize()
        out[prec] = (phi.cpu().numpy()[:, :n], coefs.cpu().numpy())
        assert rel(out[prec][0], phi_o) < 1e-5 and rel(out[prec][1], coefs_o) < 1e-5
    assert rel(out[1][0], out[0][0]) < 1e-6


def test_nlm_matlab_prox_bitexact(ops):
    """lrs_nlm_matlab_col_f32 (NLmeansfilter.m closed form, fp64; the prox of the row-split ISTA
    kernel) against the oracle's C restatement at several h (including h where the exp weights are
    tiny) and K: same evaluation order, so the only difference is exp() itself (device libm vs glibc,
    <= 1 fp64 ulp), which flips the float32 rounding of an output in ~1e-4 of the elements."""
    rng = np.random.default_rng(7)
    for K in (256, 100, 7):
        nb = 40
        g = (rng.standard_normal((nb, K)) * 0.1).astype(np.float32)
        h = np.geomspace(1e-4, 1.0, nb)
        out = ops.nlm_matlab_col(torch.from_numpy(g).cuda(), torch.from_numpy(h).cuda())
        ref = np.stack([O.nlm_matlab_col(g[j], h[j]) for j in range(nb)])
        o = out.cpu().numpy()
        np.testing.assert_array_max_ulp(o, ref, maxulp=1)
        assert np.count_nonzero(o != ref) <= 1e-3 * o.size + 1


def test_compat_pnp_ista_vs_oracle(compat_mod=None):
    """pnp_ista.m drop-in (compat.pnp_ista): NLmeansfilter prox, alpha = max eig(H^T H), h = 0.1 T;
    against the oracle's C restatement, itself pinned to a literal transcription of NLmeansfilter.m
    (tests/test_oracle.py::test_nlm_matlab_closed_form_vs_literal).  Parity vs MATLAB unpinned."""
    from lrspnp import compat
    from lrspnp.data import synthetic_dictionary
    rng = np.random.default_rng(5)
    D = synthetic_dictionary(64, 256, seed=1)
    keep = rng.random(64) > 0.1
    H = D[keep]
    y = (0.3 * rng.standard_normal(H.shape[0])).astype(np.float32)
    x = compat.pnp_ista(torch.from_numpy(y).view(-1, 1), torch.from_numpy(H), 0.1, None, 25).numpy().reshape(-1)
    a, t = O.ista_alpha_h(H, 0.1, "matlab")
    obs = keep.astype(np.uint8)
    yb = np.zeros(64, np.float32)
    yb[keep] = y
    xo = O.ista_block(yb, obs, D, a, t, 25, O.PROX_NLM_MATLAB)[0]
    # the bar of test_ista_kernel_vs_oracle: the MATLAB prox's exp(-d/h^2) weights amplify float32
    # rounding over the iterations, so the kernel may differ from the oracle by at most 4x the oracle's
    # own change under a 1-ulp perturbation of its input (and 1e-5)
    flip = np.where(rng.random(64) < 0.5, -1.0, 1.0)
    yp = (yb.astype(np.float64) * (1.0 + flip * 2.0 ** -23)).astype(np.float32)
    xp = O.ista_block(yp, obs, D, a, t, 25, O.PROX_NLM_MATLAB)[0]
    tol = max(1e-5, 4.0 * rel(xp, xo))
    assert rel(x, xo) < tol, (rel(x, xo), tol)


def test_psnr_bands_kernel_vs_oracle():
    """lrs_psnr_bands_f32 (metrics.psnr_bands / mpsnr) vs the oracle's per-band PSNR
    (main_LRS_PnP.py:379-384), including a band equal to the reference (psnr() returns 100)."""
    from lrspnp.metrics import psnr_bands
    rng = np.random.default_rng(3)
    B, H, W = 37, 29, 31
    clean = rng.random((B, H, W)).astype(np.float32)
    noisy = (clean + 0.05 * rng.standard_normal((B, H, W))).astype(np.float32)
    noisy[5] = clean[5]
    X = np.ascontiguousarray(noisy.transpose(2, 1, 0).reshape(H * W, B))    # unfold: p = i + H j
    got = psnr_bands(torch.from_numpy(X).cuda(), torch.from_numpy(clean).cuda()).cpu().numpy()
    ref = O.psnr_bands(X, clean)
    assert got[5] == 100.0
    mask = np.arange(B) != 5
    np.testing.assert_allclose(got[mask], ref[mask], rtol=1e-6)


@pytest.mark.parametrize("B,H,W", [(300, 29, 31), (37, 10, 10)])
def test_psnr_bands_wide_and_short(B, H, W):
    """lrs_psnr_bands_f32 with more bands than a workgroup has threads (B = 300) and with fewer rows
    than row slabs (P = 100), at the tolerance of test_psnr_bands_kernel_vs_oracle."""
    from lrspnp.metrics import psnr_bands
    rng = np.random.default_rng(B)
    clean = rng.random((B, H, W)).astype(np.float32)
    noisy = (clean + 0.05 * rng.standard_normal((B, H, W))).astype(np.float32)
    noisy[B - 1] = clean[B - 1]
    X = np.ascontiguousarray(noisy.transpose(2, 1, 0).reshape(H * W, B))
    got = psnr_bands(torch.from_numpy(X).cuda(), torch.from_numpy(clean).cuda()).cpu().numpy()
    ref = O.psnr_bands(X, clean)
    assert got.shape == (B,) and got[B - 1] == 100.0
    np.testing.assert_allclose(got[:B - 1], ref[:B - 1], rtol=1e-6)

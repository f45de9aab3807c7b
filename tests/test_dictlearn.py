"""Masked dictionary learning without a GPU: the fp64 checker (tests/dictlearn_ref.py) against the
theory it restates, the C ABI's argument checks (host-side: these calls never reach a device), and
the MAT v5 writer behind tools/learn_dictionary.py."""
import ctypes
import os
import sys

import numpy as np
import pytest

import dictlearn_ref as R

from lrspnp import _lib, matio

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------ checker vs theory
@pytest.mark.parametrize("seed,shape", [(0, (64, 64, 48, 150)), (1, (36, 48, 80, 60)), (2, (100, 112, 32, 300))])
def test_objective_never_rises_in_a_dictionary_step(seed, shape):
    """c = max_k sum_l |H_kl| >= lambda_max(A^T A) and the projection is onto a convex ball, so the
    majorisation-minimisation step cannot raise 1/2 ||m .* (Y - A D^T)||^2 (fp64: no slack beyond
    the last bits of the sum)."""
    n, n_pad, K, nb = shape
    Yb, ob, A, D = R.update_problem(n, n_pad, K, nb, seed)
    H, c = R.dict_stats(A)
    assert c >= np.linalg.eigvalsh(H)[-1] * (1 - 1e-12)
    Dn, obj = R.dict_step(Yb[:, :n], ob[:, :n], A, D, 25)
    assert np.all(obj[1:] <= obj[:-1] * (1 + 1e-14))
    assert obj[-1] < 0.9 * obj[0]
    assert np.all(np.linalg.norm(Dn, axis=0) <= 1 + 1e-12)
    assert np.array_equal(Dn[:, K // 3], D[:, K // 3].astype(np.float64) / max(1.0, np.linalg.norm(D[:, K // 3].astype(np.float64))))
    # float32 mode of the same arithmetic stays within the GPU tests' rounding slack
    _, o32 = R.dict_step(Yb[:, :n], ob[:, :n], A, D, 25, dtype=np.float32)
    assert np.all(o32[1:] <= o32[:-1] * (1 + 1e-6))


def test_zero_coefficients_leave_the_dictionary():
    Yb, ob, A, D = R.update_problem(64, 64, 48, 40, 3)
    Dn, obj = R.dict_step(Yb, ob, np.zeros_like(A), D, 3)
    assert np.array_equal(Dn, D.astype(np.float64)) and np.all(obj == obj[0])


PLANTED_ROUNDS = 40
# Measured with the fp64 checker (seed 0, rounds = 40, Nit = 50, n_inner = 10, lambda = 0.1): the final
# objective is PLANTED_MEASURED times the objective of the true D* coded the same way, and
# PLANTED_RECOVERED of the 32 planted atoms are recovered with |<d, d*>| > 0.99.  The bound leaves
# 10 % over the measured ratio (the checker is deterministic; the margin is for BLAS summation order).
PLANTED_MEASURED = 1.2036   # 16.9695 against 14.0991 at D* (1.0003 and 32 of 32 atoms after 100 rounds)
PLANTED_FACTOR = 1.10 * PLANTED_MEASURED
PLANTED_RECOVERED = 24


@pytest.mark.slow
def test_planted_dictionary_is_learned():
    """n = 64, K = 32, nb = 2,000, 3-sparse codes, 10 % of each block's rows masked, noise 0.01."""
    Y, obs, Ds, D0 = R.planted_problem()
    D, hist, _ = R.learn(Y, obs, D0, 0.1, 50, PLANTED_ROUNDS, 10)
    ostar = R.coded_objective(Y, obs, Ds, 0.1, 50)
    ratio, rec = hist[-1, -1] / ostar, R.recovered(D, Ds)
    print(f"planted: objective {hist[0, 0]:.6g} -> {hist[-1, -1]:.6g}, at D* {ostar:.6g}, ratio {ratio:.4f}, "
          f"{rec} of 32 atoms recovered")
    assert np.all(hist[:, 1:] <= hist[:, :-1] * (1 + 1e-14))
    assert hist[-1, -1] < PLANTED_FACTOR * ostar
    assert hist[-1, -1] < 0.05 * hist[0, 0]
    assert rec >= PLANTED_RECOVERED - 2


def test_checker_ista_matches_the_oracle():
    """The checker's ISTA restates ista.m:15-23 as oracle/lrs_oracle.c does (float32 mode against the
    oracle's float32 iterates with fp64-accumulated products)."""
    from oracle import oracle as O
    Y, obs, _, D0 = R.planted_problem(nb=40, seed=5)
    alpha, thr = R.ista_alpha_soft(D0, obs, 0.1, np.float32)
    for j in range(0, 40, 7):
        a, t = O.ista_alpha_h(D0[obs[j].astype(bool)], 0.1, "soft")
        assert abs(alpha[j] - a) <= 4e-7 * a and abs(thr[j] - t) <= 4e-7 * t
    X = R.ista_soft(Y, obs, D0, alpha, thr, 30, dtype=np.float32)
    Xo, _ = O.ista_batch(Y, obs, D0, alpha.astype(np.float32), thr.astype(np.float64), 30, O.PROX_SOFT)
    assert np.linalg.norm(X - Xo) <= 1e-5 * np.linalg.norm(Xo)


# ------------------------------------------------------------------------------------ ABI checks
def test_abi_argument_checks():
    L = _lib.lib()
    assert L.lrs_version().startswith(b"lrspnp-hip 0.2")
    n, n_pad, K, nb = 100, 112, 48, 37
    ws = L.lrs_dict_workspace(n, n_pad, K, nb)
    assert ws >= nb * n_pad * 4 + n * K * 4
    assert L.lrs_dict_workspace(1296, 1296, 512, 65536) > 0
    for bad in [(n, n_pad, 513, nb), (n, 100, K, nb), (n, 96, K, nb), (0, n_pad, K, nb), (n, n_pad, K, 0),
                (n, n_pad, K, (1 << 24) + 1)]:
        assert L.lrs_dict_workspace(*bad) == 0, bad
    fake = ctypes.c_void_p(4096)   # never dereferenced: every check below comes before a launch
    upd = lambda n_, np_, K_, nb_, obj, wsb, ni=1: L.lrs_dict_update_f32(fake, fake, fake, fake, n_, np_, K_, nb_, fake,
                                                                         ni, obj, fake, wsb, None)
    assert upd(n, n_pad, 513, nb, fake, ws) == -2                    # LRS_E_UNSUPPORTED
    assert upd(n, n_pad, K, (1 << 24) + 1, fake, ws) == -2
    assert upd(n, n_pad, K, nb, fake, ws - 1) == -3                  # LRS_E_WORKSPACE
    assert upd(n, n_pad, K, nb, None, ws) == -1                      # LRS_E_INVALID: null obj
    assert upd(n, 100, K, nb, fake, ws) == -1                        # n_pad % 16
    assert upd(n, n_pad, K, nb, fake, ws, ni=-1) == -1
    assert L.lrs_dict_update_f32(fake, fake, fake, fake, n, n_pad, K, nb, fake, 1, fake, None, ws, None) == -3
    assert L.lrs_dict_stats_f32(fake, nb, 513, fake, fake, fake, ws, None) == -2
    assert L.lrs_dict_stats_f32(fake, nb, K, None, fake, fake, ws, None) == -1
    assert L.lrs_dict_stats_f32(fake, nb, K, fake, None, fake, ws, None) == -1
    assert L.lrs_dict_stats_f32(fake, nb, K, fake, fake, fake, 16, None) == -3
    assert L.lrs_dict_normalise_f32(None, n, K, None) == -1
    assert L.lrs_dict_normalise_f32(fake, n, 513, None) == -2


def test_package_exports_and_config_defaults():
    import lrspnp
    from lrspnp import DictLearnConfig, LrsPnPConfig, learn_dictionary  # noqa: F401
    from lrspnp.dictlearn import warm_start_supported
    c = DictLearnConfig()
    assert (c.K, c.bb, c.train_sliding, c.max_blocks, c.lambda_ista, c.Nit, c.rounds, c.n_inner, c.normalise,
            c.seed) == (256, 36, None, 65536, 0.1, 100, 20, 10, True, 0)
    assert LrsPnPConfig().dict_cfg is None
    assert lrspnp.ops.dict_stats and lrspnp.ops.dict_update
    # the dictionary-resident kernels (n_pad <= 64, K = 256) cold-start; every other path continues
    assert not warm_start_supported(64, 256, False)
    assert warm_start_supported(64, 32, False) and warm_start_supported(1296, 256, False)
    assert warm_start_supported(64, 256, True)


# ----------------------------------------------------------------------------------------- matio
def test_mat5_writer_roundtrip(tmp_path):
    scipy_io = pytest.importorskip("scipy.io")
    rng = np.random.default_rng(0)
    D = rng.standard_normal((1296, 7)).astype(np.float32)
    h = rng.random((3, 11))
    p = matio.save_mat5(str(tmp_path / "trained_dictionary.mat"), {"Dictionary": D, "history": h, "v": np.arange(5)})
    assert matio.mat_version(p) == "v5"
    got = matio.load_mat(p)
    assert list(got) == ["Dictionary", "history", "v"]
    assert got["Dictionary"].dtype == np.float32 and np.array_equal(got["Dictionary"], D)
    assert got["history"].dtype == np.float64 and np.array_equal(got["history"], h)
    assert np.array_equal(got["v"], np.arange(5, dtype=np.float64)[None])
    # what main_LRS_PnP.py:159-160 does with the file
    assert np.array_equal(scipy_io.loadmat(p)["Dictionary"], D)
    with pytest.raises(ValueError):
        matio.save_mat5(str(tmp_path / "x.mat"), {"": D})


def test_tool_reads_inputs_and_writes_both_files(tmp_path):
    """tools/learn_dictionary.py: its loaders and writers (the training itself needs the GPU)."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import learn_dictionary as T
    finally:
        sys.path.pop(0)
    rng = np.random.default_rng(1)
    cube = rng.random((5, 6, 6)).astype(np.float32)
    mask = (rng.random((6, 6)) > 0.2).astype(np.uint8)
    np.savez(tmp_path / "cube.npz", img=cube)
    matio.save_mat5(str(tmp_path / "mask.mat"), {"msk": mask[None, None]})
    assert np.array_equal(T.load_cube(str(tmp_path / "cube.npz"), None, False), cube)
    assert np.array_equal(T.load_cube(str(tmp_path / "cube.npz"), "img", True), cube.transpose(2, 0, 1))
    assert np.array_equal(T.load_mask(str(tmp_path / "mask.mat"), "msk", (6, 6)), mask.astype(np.float32))
    with pytest.raises(SystemExit):
        T.load_mask(str(tmp_path / "mask.mat"), "msk", (5, 6))
    D = rng.standard_normal((36, 4)).astype(np.float32)
    npz, mat = T.save(str(tmp_path / "out"), D, np.ones((2, 3)))
    assert np.array_equal(np.load(npz)["Dictionary"], D)
    assert np.array_equal(matio.load_mat(mat)["Dictionary"], D)

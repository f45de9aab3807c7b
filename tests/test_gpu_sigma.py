"""GPU: the spectral-norm chain (k_sn_gram, k_sn_gram_reduce, k_sn_sigma, k_sn_apply through
lrs_sigma_max_f32 and lrspnp.dip.sigma_max) against numpy's fp64 SVD of the same float32 matrices.

The matrices are tests/sn_emu.py's (families A to F); tests/test_sn_emu.py shows on the CPU
that a faithful model of the chain is within one float32 ulp on every case of A to E and that six degraded
chains are not.  Per case: rtol 2e-6 against the SVD, |sigma - float32(ref)| <= spacing(float32(ref)), and
scale == max(1, sigma32 / lambda) in float32 exactly.  Family F always asserts sigma_2 (1 - ulp) <= sigma
<= sigma_1 (1 + ulp), and one ulp wherever the recorded verdict of the model (tests/golden/
sn_f_verdicts.json) is "within one ulp".
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import sn_emu as E  # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
OK, E_INVALID, E_UNSUPPORTED, E_WORKSPACE = 0, -1, -2, -3


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lrspnp import _lib
    return _lib.device_lib()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def raw(L, mats, lam=1.0, wn=False, ws=None, short=0, fill=None):
    """lrs_sigma_max_f32 on device copies of the float32 matrices; returns (rc, sigma, scale, W after, Wn)."""
    n = len(mats)
    dev = [torch.from_numpy(np.ascontiguousarray(m)).cuda() for m in mats]
    out = [torch.full_like(d, 7.0) for d in dev] if wn else None
    W = (ctypes.c_void_p * n)(*[d.data_ptr() for d in dev])
    Wn = (ctypes.c_void_p * n)(*[o.data_ptr() for o in out]) if wn else None
    rows = (ctypes.c_int * n)(*[m.shape[0] for m in mats])
    cols = (ctypes.c_int * n)(*[m.shape[1] for m in mats])
    sig = torch.full((max(n, 1),), -5.0, device="cuda")
    sc = torch.full((max(n, 1),), -5.0, device="cuda")
    nb = int(L.lrs_sigma_max_workspace(n))
    if ws is None:
        ws = torch.zeros(max(nb, 1), dtype=torch.uint8, device="cuda")
        if fill is not None:
            ws.fill_(fill)
    rc = L.lrs_sigma_max_f32(W, Wn, rows, cols, n, ctypes.c_float(lam), _ptr(sig), _ptr(sc), _ptr(ws), nb - short,
                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, sig.cpu().numpy()[:n], sc.cpu().numpy()[:n], [d.cpu().numpy() for d in dev], \
        [o.cpu().numpy() for o in out] if wn else None


@functools.lru_cache(maxsize=None)
def refs(family):
    cases = {"A": E.family_a, "B": E.family_b, "C": E.family_c, "D": E.family_d, "E": E.family_e,
             "F": E.family_f}[family]()
    return cases, {k: E.sigma_ref(W) for k, W in cases.items()}


def check(names, sig, sc, ref, lam=1.0):
    """The three assertions of a contract case, for a batch; every figure is printed first."""
    r = np.array([ref[k][0] for k in names])
    r32 = r.astype(np.float32)
    ulps = [E.ulp_err(s, x) for s, x in zip(sig, r)]
    for k, s, x, u in zip(names, sig, r, ulps):
        print(f"{k}: sigma {s!r} ref {x!r} ulp {u:+.2f}")
    np.testing.assert_allclose(sig.astype(np.float64), r, rtol=2e-6, atol=0.0)
    assert (np.abs(sig - r32) <= np.spacing(r32)).all(), dict(zip(names, ulps))
    want = np.array([E.scale_of(s, lam) for s in sig], np.float32)
    assert sc.tobytes() == want.tobytes(), (sc, want)


@pytest.mark.parametrize("family", ["A", "B", "C", "D", "E"])
def test_family(L, family):
    cases, ref = refs(family)
    names = list(cases)
    for i in range(0, len(names), 40):
        part = names[i:i + 40]
        rc, sig, sc, _, _ = raw(L, [cases[k] for k in part])
        assert rc == OK
        assert np.isfinite(sig).all()
        check(part, sig, sc, ref)


def test_sigma_max_wrapper():
    from lrspnp.dip import sigma_max
    cases, ref = refs("A")
    names = list(cases)
    for lam in (1.0, 0.5):
        sig, sc = sigma_max([torch.from_numpy(cases[k]).cuda() for k in names], ln_lambda=lam)
        check(names, sig.cpu().numpy(), sc.cpu().numpy(), ref, lam)


def test_scale_batch_independent(L):
    """Batch position and companions change no sigma bitwise."""
    cases, ref = refs("D")
    comp = E.d_companions()
    alone = {k: raw(L, [W])[1][0] for k, W in {**cases, **comp}.items()}
    names = ["7x3"] + list(cases) + ["198x128"]
    rc, sig, sc, _, _ = raw(L, [{**cases, **comp}[k] for k in names])
    assert rc == OK
    assert sig.tobytes() == np.array([alone[k] for k in names], np.float32).tobytes()
    rc, sig2, _, _, _ = raw(L, [{**cases, **comp}[k] for k in names[::-1]])
    assert sig2.tobytes() == sig[::-1].tobytes()
    i = [names.index(k) for k in cases]
    check(list(cases), sig[i], sc[i], ref)


def test_start_vector_alignment(L):
    """Family F.  Never above sigma_1 nor below sigma_2 by more than an ulp; one ulp wherever the model is.
    Where the model settles on sigma_2 (component below c(g)) that bound is the guarantee.
    Measured: the kernel equals the model on all 16 cases (low by 84, 8388.5, 839 and 84 ulp on c1e-05_g1e-05,
    c0_g0.001, c0_g0.0001, c0_g1e-05)."""
    cases, ref = refs("F")
    with open(os.path.join(HERE, "golden", "sn_f_verdicts.json")) as f:
        verdict = json.load(f)
    names = list(cases)
    rc, sig, sc, _, _ = raw(L, [cases[k] for k in names])
    assert rc == OK
    for k, s in zip(names, sig):
        s1, s2 = (np.float32(x) for x in ref[k])
        print(f"{k}: ulp {E.ulp_err(s, ref[k][0]):+.2f} (model {verdict[k]['model_ulp']:+.2f})")
        assert s <= s1 + np.spacing(s1), k
        assert s >= s2 - np.spacing(s2), k
        if verdict[k]["within_1ulp"]:
            assert abs(s - s1) <= np.spacing(s1), k
            assert abs(float(s) - ref[k][0]) <= 2e-6 * ref[k][0], k
    want = np.array([E.scale_of(s, 1.0) for s in sig], np.float32)
    assert sc.tobytes() == want.tobytes()


@pytest.mark.parametrize("lam", [0.5, 1.0, 2.0])
def test_apply_and_state(L, lam):
    """Wn = float32 W / scale bitwise, W unchanged, Wn = NULL leaves sigma the same, two runs equal."""
    mats = [E.gaussian(128, 1152, 6000, 0.04), E.gaussian(198, 128, 6001, 0.1), E.gaussian(7, 3, 6002),
            E.gaussian(64, 64, 6003, 0.01), np.zeros((5, 9), np.float32)]
    rc, sig, sc, Wa, Wn = raw(L, mats, lam, wn=True)
    assert rc == OK
    want = np.array([E.scale_of(s, lam) for s in sig], np.float32)
    assert sc.tobytes() == want.tobytes()
    assert (sc > 1.0).any() and (sc == 1.0).any()
    for m, wa, wn, s in zip(mats, Wa, Wn, sc):
        assert wa.tobytes() == m.tobytes()
        assert wn.tobytes() == (m / np.float32(s)).astype(np.float32).tobytes()
    rc, sig0, sc0, _, _ = raw(L, mats, lam)
    assert rc == OK and sig0.tobytes() == sig.tobytes() and sc0.tobytes() == sc.tobytes()
    rc, sig1, sc1, _, _ = raw(L, mats, lam, wn=True)
    assert sig1.tobytes() == sig.tobytes() and sc1.tobytes() == sc.tobytes()


def test_workspace_state(L):
    """A workspace of 0xFF bytes, and a 7 x 3 matrix after a 128 x 1152 one in the same workspace, give the
    bits of a fresh zeroed workspace; n = 1 and n = 40 work."""
    big, small = E.gaussian(128, 1152, 6000, 0.04), E.gaussian(7, 3, 6002)
    fresh_big, fresh_small = raw(L, [big])[1], raw(L, [small])[1]
    assert raw(L, [big], fill=0xFF)[1].tobytes() == fresh_big.tobytes()
    assert raw(L, [small], fill=0xFF)[1].tobytes() == fresh_small.tobytes()
    ws = torch.zeros(int(L.lrs_sigma_max_workspace(1)), dtype=torch.uint8, device="cuda")
    assert raw(L, [big], ws=ws)[1].tobytes() == fresh_big.tobytes()
    assert raw(L, [small], ws=ws)[1].tobytes() == fresh_small.tobytes()
    mats = [E.gaussian(3 + i, 40 - i, 6100 + i) for i in range(40)]
    rc, sig, sc, _, _ = raw(L, mats, fill=0xFF)
    assert rc == OK
    ref = {str(i): E.sigma_ref(m) for i, m in enumerate(mats)}
    check([str(i) for i in range(40)], sig, sc, ref)


def test_refusals(L):
    ok = [E.gaussian(8, 8, 1)]
    assert raw(L, [np.zeros((129, 129), np.float32)])[0] == E_UNSUPPORTED
    assert raw(L, [np.zeros((129, 400), np.float32)])[0] == E_UNSUPPORTED
    for lam in (0.0, -1.0, float("nan")):
        rc, sig, sc, _, _ = raw(L, ok, lam)
        assert rc == E_INVALID and sig[0] == -5.0 and sc[0] == -5.0
    rc, sig, _, _, _ = raw(L, ok, short=1)
    assert rc == E_WORKSPACE and sig[0] == -5.0
    # n = 0: OK, nothing touched (every pointer NULL)
    assert L.lrs_sigma_max_f32(None, None, None, None, 0, ctypes.c_float(1.0), None, None, None, 0, None) == OK
    # a NULL W[i] and a non-positive dimension
    d = torch.zeros(64, device="cuda")
    sig = torch.full((2,), -5.0, device="cuda")
    ws = torch.zeros(int(L.lrs_sigma_max_workspace(2)), dtype=torch.uint8, device="cuda")
    for W, r, c in (((d.data_ptr(), None), (8, 8), (8, 8)), ((d.data_ptr(), d.data_ptr()), (8, 0), (8, 8)),
                    ((d.data_ptr(), d.data_ptr()), (8, 8), (8, -3))):
        rc = L.lrs_sigma_max_f32((ctypes.c_void_p * 2)(*W), None, (ctypes.c_int * 2)(*r), (ctypes.c_int * 2)(*c), 2,
                                 ctypes.c_float(1.0), _ptr(sig), _ptr(sig), _ptr(ws), ws.numel(), None)
        assert rc == E_INVALID
    torch.cuda.synchronize()
    assert (sig.cpu().numpy() == -5.0).all()


def test_non_finite_weights(L):
    """A NaN and an Inf matrix beside two finite ones: the call returns, the finite sigmas are bitwise what
    they are alone, the others are non-finite or zero with scale = fmaxf(1, sigma / lambda).

    Every loop of the three kernels is bounded whatever the operands: the Gram's run over the inner range
    and fixed tile counts; k_sn_sigma's Lanczos loop is `k < m` (a NaN beta leaves it through the
    !(b > ...) break), sn_multisect is `it < 12`, both Sturm loops run over `n` terms, and sn_round is one
    barrier with an integer atomicMax; no loop waits on a floating-point comparison."""
    fin = [E.gaussian(128, 300, 6200, 0.05), E.gaussian(20, 9, 6201)]
    nan = E.gaussian(128, 300, 6202, 0.05)
    nan[17, 100] = np.nan
    inf = E.gaussian(64, 128, 6203, 0.05)
    inf[3, 5] = np.inf
    alone = raw(L, fin)[1]
    rc, sig, sc, _, _ = raw(L, [fin[0], nan, inf, fin[1]], 0.5)
    assert rc == OK
    assert sig[[0, 3]].tobytes() == alone.tobytes()
    for s in sig[1:3]:
        assert not np.isfinite(s) or s == 0.0
    want = np.array([E.scale_of(s, 0.5) for s in sig], np.float32)
    assert np.array_equal(sc, want, equal_nan=True), (sig, sc, want)

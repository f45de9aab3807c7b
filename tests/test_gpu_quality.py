"""The quality monitor on the MI355X: ops.cube_quality (lrs_cube_quality_f32) against tests/quality_ref.py, the
fp64 restatement of its definitions; ops.keep_best (lrs_keep_best_f32) against the restated rule, bit for bit;
LrsPnP.run() against a solver stepped by hand.

The bounds come from the arithmetic, not from the kernel: every sum here has fewer than 2^19 terms (70001 * 4 at
the most), each the fp64 image of a float32 product or square and none negative, so kernel and restatement differ
by the rounding of two summation orders, at most 2^19 * 2^-53 ~ 6e-11 relative.  sse_b and the relative error are held to 1e-10
relative; a PSNR is 5 log10 of such a ratio, so 1e-9 absolute is wider still; SAM to 1e-9 rad, which needs the
true angles away from 0 (d angle <= d cos / sin(angle): at angle >= 1e-3 a 1e-15 cosine error is 1e-12 rad), and
the test asserts that on the restatement.  With one band the cosine of two positive numbers is exactly 1 in
both (x c / (sqrt(x^2) sqrt(c^2)) has no rounding), so the angle is exactly 0 there."""
import ctypes

import numpy as np
import pytest
import torch

import quality_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (7, 3), (64, 1), (300, 5), (257, 64), (130, 65), (1000, 198), (50, 513), (70001, 4),
          (33, 300)]   # the last: 257..512 bands, the widest register form, which the others do not reach
REGIONS = ["none", "half", "hole", "zero_band", "zero"]
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3


@pytest.fixture(scope="module")
def ops():
    from lrspnp import ops as o
    o.device_lib()
    return o


def _inputs(P, B):
    rng = np.random.default_rng(1000 * P + B)
    return rng.random((P, B), dtype=np.float32), rng.random((P, B), dtype=np.float32)


def _region(kind, P, B):
    rng = np.random.default_rng(7 * P + B)
    if kind == "none":
        return None
    if kind == "half":
        return (rng.random((P, B)) < 0.5).astype(np.uint8)
    if kind == "hole":   # 1 - M of a pixel mask: whole spectra
        return np.repeat((rng.random((P, 1)) < 0.3).astype(np.uint8), B, axis=1)
    r = np.ones((P, B), np.uint8)
    if kind == "zero_band":
        r[:, B // 2] = 0
        return r
    return np.zeros((P, B), np.uint8)


_REF = {}


def _ref(P, B, kind):
    """The restatement of one case, computed once and shared."""
    if (P, B, kind) not in _REF:
        X, C = _inputs(P, B)
        ref = R.cube_quality(X, C, _region(kind, P, B))
        for v in ref.values():
            v.setflags(write=False)
        _REF[(P, B, kind)] = ref
    return _REF[(P, B, kind)]


def _d(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(ops, X, C, reg):
    q = torch.full((4,), -7.0, dtype=torch.float64, device="cuda")
    pb = torch.full((X.shape[1],), -7.0, dtype=torch.float64, device="cuda")
    ops.cube_quality(X, C, reg, q=q, psnr_bands=pb)
    torch.cuda.synchronize()
    return q.cpu().numpy(), pb.cpu().numpy()


def _close_nan(got, want, atol=0.0, rtol=0.0):
    """NaN exactly where want has NaN; elsewhere |got - want| <= atol + rtol |want|.  Returns the largest error."""
    got, want = np.atleast_1d(got), np.atleast_1d(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok])
    assert (err <= atol + rtol * np.abs(want[ok])).all(), (got, want)
    return err.max() if ok.any() else 0.0


@pytest.mark.parametrize("P,B", SHAPES)
def test_parity_with_the_restatement(ops, P, B):
    Xh, Ch = _inputs(P, B)
    X, C = _d(Xh), _d(Ch)
    for kind in REGIONS:
        ref = _ref(P, B, kind)
        # the premise of the SAM bound, on the restatement: no counted pixel's angle is near 0 (one band: exactly 0)
        if B == 1:
            assert (ref["angles"] == 0.0).all()
        else:
            assert (ref["angles"] >= 1e-3).all(), (kind, ref["angles"].min())
        q, pb = _run(ops, X, C, _d(_region(kind, P, B)))
        e_pb = _close_nan(pb, ref["psnr_bands"], atol=1e-9)
        e_mp = _close_nan(q[0], ref["q"][0], atol=1e-9)
        e_sam = _close_nan(np.radians(q[1]), np.radians(ref["q"][1]), atol=1e-9)
        e_rel = _close_nan(q[2], ref["q"][2], rtol=1e-10)
        # sse_b itself, back out of the band PSNR: 255^2 n_b / 10^(psnr / 5), to 1e-10 relative
        live = ~np.isnan(ref["psnr_bands"])
        sse = 255.0 ** 2 * ref["n_b"][live] / 10.0 ** (pb[live] / 5.0)
        e_sse = np.abs(sse / ref["sse_b"][live] - 1).max() if live.any() else 0.0
        print(f"({P},{B}) {kind}: psnr_b {e_pb:.2e} mpsnr {e_mp:.2e} sam {e_sam:.2e} rad rel_err {e_rel:.2e} "
              f"sse_b {e_sse:.2e} rel")
        assert e_sse <= 1e-10, (kind, e_sse)
        assert q[3] == ref["q"][3], (kind, q[3], ref["q"][3])


@pytest.mark.parametrize("P,B", [(7, 3), (1000, 198), (50, 513)])
def test_identical_cubes(ops, P, B):
    C = _d(_inputs(P, B)[1] + np.float32(0.01))
    q, pb = _run(ops, C.clone(), C, None)
    assert (pb == 100.0).all() and q[0] == 100.0
    assert 0.0 <= np.radians(q[1]) <= 1e-6
    assert q[2] == 0.0 and q[3] == P


def test_scaled_and_orthogonal_spectra(ops):
    C = _d(_inputs(40, 6)[1] + np.float32(0.01))
    q, _ = _run(ops, 2 * C, C, None)
    assert np.radians(q[1]) <= 1e-6 and abs(q[2] - 1.0) <= 1e-10
    X = torch.zeros(9, 4, device="cuda")
    Z = torch.zeros(9, 4, device="cuda")
    X[:, 0], Z[:, 3] = 0.5, 0.25
    q, _ = _run(ops, X, Z, None)
    assert abs(q[1] - 90.0) <= np.degrees(1e-9) and q[3] == 9


@pytest.mark.parametrize("P,B", [(300, 5), (130, 65), (50, 513)])
def test_zero_norm_spectra_are_skipped(ops, P, B):
    Xh, Ch = (a.copy() for a in _inputs(P, B))
    Xh[3], Xh[P - 1], Ch[10], Ch[3] = 0, 0, 0, 0     # row 3 in both
    ref = R.cube_quality(Xh, Ch)
    assert ref["q"][3] == P - 3
    q, pb = _run(ops, _d(Xh), _d(Ch), None)
    assert q[3] == P - 3
    _close_nan(np.radians(q[1]), np.radians(ref["q"][1]), atol=1e-9)
    _close_nan(pb, ref["psnr_bands"], atol=1e-9)
    # a region that leaves only zero-norm pixels: no SAM, but the other scores live on
    reg = np.zeros((P, B), np.uint8)
    reg[10] = 1
    ref = R.cube_quality(Xh, Ch, reg)
    q, _ = _run(ops, _d(Xh), _d(Ch), _d(reg))
    assert q[3] == 0 and np.isnan(q[1]) and np.isnan(ref["q"][1])
    _close_nan(q[0], ref["q"][0], atol=1e-9)
    assert np.isnan(q[2]) and np.isnan(ref["q"][2])   # sum r c^2 = 0: row 10 of C is zero


@pytest.mark.parametrize("P,B", [(300, 5), (1000, 198), (50, 513)])
def test_reruns_and_a_misaligned_base_give_the_same_bits(ops, P, B):
    Xh, Ch = _inputs(P, B)
    for kind in ("none", "half"):
        rh = _region(kind, P, B)
        X, C, reg = _d(Xh), _d(Ch), _d(rh)
        bits = lambda qp: (qp[0].view(np.int64).copy(), qp[1].view(np.int64).copy())
        q0, p0 = bits(_run(ops, X, C, reg))
        q1, p1 = bits(_run(ops, X, C, reg))
        assert np.array_equal(q0, q1) and np.array_equal(p0, p1)
        # the same data one float (region: one byte) further on
        Xo = torch.empty(P * B + 1, device="cuda")[1:].view(P, B).copy_(X)
        Co = torch.empty(P * B + 1, device="cuda")[1:].view(P, B).copy_(C)
        ro = None if reg is None else torch.empty(P * B + 1, dtype=torch.uint8, device="cuda")[1:].view(P, B).copy_(reg)
        assert Xo.data_ptr() % 8 == 4 and Co.data_ptr() % 8 == 4
        q2, p2 = bits(_run(ops, Xo, Co, ro))
        assert np.array_equal(q0, q2) and np.array_equal(p0, p2)


def test_refusals_write_nothing(ops):
    from lrspnp._lib import device_lib
    L = device_lib()
    P, B = 40, 6
    X, C = (_d(a) for a in _inputs(P, B))
    ws = ops.cube_quality_workspace(P, B, "cuda")
    q = torch.full((4,), -7.0, dtype=torch.float64, device="cuda")
    vp = ctypes.c_void_p
    ok = dict(X=vp(X.data_ptr()), C=vp(C.data_ptr()), P=P, B=B, q=vp(q.data_ptr()), ws=vp(ws.data_ptr()),
              wsb=ws.numel())

    def call(**kw):
        a = dict(ok, **kw)
        return L.lrs_cube_quality_f32(a["X"], a["C"], None, a["P"], a["B"], a["q"], None, a["ws"], a["wsb"], None)

    for k in ("X", "C", "q", "ws"):
        assert call(**{k: None}) == INVALID, k
    for k in ("P", "B"):
        assert call(**{k: 0}) == INVALID and call(**{k: -3}) == INVALID, k
    assert call(wsb=ws.numel() - 1) == WORKSPACE and call(wsb=0) == WORKSPACE
    big = (1 << 63) - 1
    assert call(P=1 << 31, B=1, wsb=big) == UNSUPPORTED and call(P=1 << 20, B=1 << 11, wsb=big) == UNSUPPORTED
    assert call(P=(1 << 31) - 1, B=1, wsb=0) == WORKSPACE          # the last size served: only the workspace is short
    assert L.lrs_cube_quality_workspace(1 << 31, 1) == 0 and L.lrs_cube_quality_workspace(0, 4) == 0
    # keep_best's refusals
    best = torch.full((2,), float("nan"), dtype=torch.float64, device="cuda")
    src, dst = torch.ones(8, device="cuda"), torch.zeros(8, device="cuda")
    kb = dict(score=vp(q.data_ptr()), sign=1, src=vp(src.data_ptr()), dst=vp(dst.data_ptr()), n=8,
              best=vp(best.data_ptr()))

    def keep(**kw):
        a = dict(kb, **kw)
        return L.lrs_keep_best_f32(a["score"], a["sign"], 0, a["src"], a["dst"], a["n"], a["best"], None)

    for k in ("score", "src", "dst", "best"):
        assert keep(**{k: None}) == INVALID, k
    for s in (0, 2, -2, 7):
        assert keep(sign=s) == INVALID, s
    assert keep(n=0) == INVALID and keep(n=-1) == INVALID
    assert keep(dst=vp(src.data_ptr())) == INVALID                      # aliased
    assert keep(dst=vp(src.data_ptr() + 16), n=8) == INVALID            # overlapping
    torch.cuda.synchronize()
    assert (q == -7.0).all() and torch.isnan(best).all() and (dst == 0).all()
    assert call() == 0 and keep(sign=-1) == 0                           # and the unrefused calls run
    torch.cuda.synchronize()
    assert not (q == -7.0).any() and (dst == 1).all()


def _bits(t):
    return t.view(torch.int64)


@pytest.mark.parametrize("n", [1, 255, 1000003])
@pytest.mark.parametrize("sign", [1, -1])
def test_keep_best_follows_the_rule(ops, n, sign):
    nan = float("nan")
    scores = [nan, 3.0, 3.0, nan, 5.0, 4.0, 5.0, -1.0, nan, 7.5, -2.0]   # NaN start, ties, both directions
    g = torch.Generator(device="cuda").manual_seed(n)
    snaps = [torch.rand(n, device="cuda", generator=g) for _ in scores]
    want = R.keep_best(scores, sign, list(range(len(scores))))
    assert len({w[2] for w in want}) >= 3                                 # the script does switch snapshots
    sentinel = torch.full((n,), -3.0, device="cuda")
    dst = sentinel.clone()
    best = torch.full((2,), nan, dtype=torch.float64, device="cuda")
    score = torch.empty(1, dtype=torch.float64, device="cuda")
    for t, s in enumerate(scores):
        score.fill_(s)
        before = best.clone()
        ops.keep_best(score, sign, t, snaps[t], dst, best)
        torch.cuda.synchronize()
        w_score, w_it, held = want[t]
        expect = torch.tensor([w_score, w_it], dtype=torch.float64, device="cuda")
        assert torch.equal(_bits(best), _bits(expect)) or (np.isnan(w_score) and torch.isnan(best).all()), (t, best)
        if held != t:                                                     # not better: nothing is written
            assert torch.equal(_bits(best), _bits(before)), t
        assert torch.equal(dst, sentinel if held is None else snaps[held]), (t, held)


def test_keep_best_on_unaligned_buffers(ops):
    """Bases that are not 16-byte aligned take the kernel's scalar copy."""
    n = 1021
    src = torch.rand(n + 1, device="cuda")[1:]
    dst = torch.zeros(n + 3, device="cuda")[3:]
    best = torch.full((2,), float("nan"), dtype=torch.float64, device="cuda")
    ops.keep_best(torch.tensor([2.5], dtype=torch.float64, device="cuda"), -1, 4, src, dst, best)
    torch.cuda.synchronize()
    assert torch.equal(dst, src) and best.tolist() == [2.5, 4.0]


# ---- LrsPnP.run() ------------------------------------------------------------------------------------------
H, W, NB = 12, 10, 8
NORM_RTOL = 6 * 2.0 ** -53


def _solver(lowrank):
    from lrspnp import LrsPnP, LrsPnPConfig, NlmCubeConfig
    from lrspnp.data import mask_matrix, synthetic_cube, synthetic_dictionary, unfold
    obs, clean, _ = synthetic_cube(H, W, NB, seed=3)
    pix = (np.random.default_rng(0).random((H, W)) > 0.2).astype(np.float32)
    M = mask_matrix(pix, NB)
    cfg = LrsPnPConfig(lowrank=lowrank, nlm=NlmCubeConfig(3, 2, 0.1, 0.0), bb=4, sliding=4, Nit=10)
    s = LrsPnP(unfold(obs) * M, M, synthetic_dictionary(16, 64, 0), cfg, image_shape=(H, W))
    return s, np.ascontiguousarray(clean, dtype=np.float32), M


@pytest.mark.parametrize("lowrank", ["svt", "nlm"])
def test_run_against_a_solver_stepped_by_hand(lowrank):
    from lrspnp import metrics
    from lrspnp.data import unfold
    from lrspnp.solver import HISTORY_COLUMNS
    n_iter = 6
    hand, clean, M = _solver(lowrank)
    clean_d = torch.from_numpy(clean).cuda()
    Xs, norms, mps = [], [], []
    for _ in range(n_iter):
        hand.step()
        Xs.append(hand.X.clone())
        norms.append(hand.norms.cpu().numpy().copy())
        mps.append(float(metrics.psnr_bands(hand.X, clean_d).mean()))
    torch.cuda.synchronize()

    for region, clean_arg in (("hole", clean), ("all", unfold(clean))):     # both layouts of clean
        s, _, _ = _solver(lowrank)
        hist = s.run(n_iter, clean_arg, region=region, keep_best="mpsnr")
        assert hist.dtype.names == HISTORY_COLUMNS and hist.shape == (n_iter,)
        for name, t in (("X", hand.X), ("L1", hand.L1), ("L2", hand.L2)):
            assert torch.equal(getattr(s, name), t), (region, name)
        # the sums of admm_update's workgroups meet in fp64 atomics, whose order is not fixed: this cube (960 entries)
        # has 4 workgroups, so either solver's sum is within 3 roundings of the exact one and the two within 6
        got = np.stack([hist.norm_dX, hist.norm_dL1, hist.norm_dL2], axis=1)
        np.testing.assert_allclose(got, np.stack(norms), rtol=NORM_RTOL, atol=0)
        reg = None if region == "all" else (M == 0).astype(np.uint8)
        for t in range(n_iter):
            ref = R.cube_quality(Xs[t].cpu().numpy(), unfold(clean), reg)["q"]
            assert abs(hist.mpsnr[t] - ref[0]) <= 1e-9 and abs(hist.rel_err[t] - ref[2]) <= 1e-10 * ref[2]
            assert abs(np.radians(hist.sam_deg[t]) - np.radians(ref[1])) <= 1e-9
        if region == "all":
            assert np.abs(hist.mpsnr - np.array(mps)).max() <= 1e-9
        k = int(np.argmax(hist.mpsnr))                                   # the first of equals
        assert s.best_iteration == k and s.best_score == hist.mpsnr[k]
        assert torch.equal(s.best_X, Xs[k]), (region, k)

    # a run in which no iteration has a score keeps nothing, and still steps
    s, _, _ = _solver(lowrank)
    s.run(3, clean, region=np.zeros((NB, H, W)), keep_best="rel_err")    # an empty region: every score NaN
    assert s.best_X is None and s.best_iteration is None and s.best_score is None
    assert torch.equal(s.X, Xs[2])


def test_run_without_clean_and_its_refusals():
    from lrspnp import LrsError
    s, clean, _ = _solver("svt")
    hand, _, _ = _solver("svt")
    hist = s.run(3)
    norms = []
    for _ in range(3):
        hand.step()
        norms.append(hand.norms.cpu().numpy().copy())
    assert torch.equal(s.X, hand.X)
    assert np.isnan(hist.mpsnr).all() and np.isnan(hist.sam_deg).all() and np.isnan(hist.rel_err).all()
    np.testing.assert_allclose(np.stack([hist.norm_dX, hist.norm_dL1, hist.norm_dL2], axis=1), np.stack(norms),
                               rtol=NORM_RTOL, atol=0)
    assert s.best_X is None and s.best_iteration is None
    before = s.X.clone()
    for kw in (dict(keep_best="mpsnr"), dict(clean=clean, keep_best="psnr"), dict(clean=clean, region="holes"),
               dict(clean=clean[:, :, :5]), dict(clean=clean, region=np.ones((3, 3)))):
        with pytest.raises(LrsError):
            s.run(2, **kw)
    with pytest.raises(LrsError):
        s.run(0, clean)
    s.comm = object()                                                    # a row-slab shard is refused
    with pytest.raises(LrsError, match="comm"):
        s.run(2, clean)
    assert torch.equal(s.X, before)                                      # a refused run() has not stepped

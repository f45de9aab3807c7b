"""GPU: the TV term of the DIP output (csrc/dip_tv.h: lrs_sstv_f32, ops.sstv).

The kernel against tests/sstv_ref.py (fp64 closed form): every weight alone and all three, eps = 0 on grid
inputs with ties and eps = 1e-3 on random inputs, shapes with C, H or W = 1, several workgroups, the float4 and
the scalar form; accumulation into gout and the loss, the frame, determinism, refusals.

Tolerances.  Gradient, eps = 0, grid inputs: |err| <= 2^-20 (4 w_sp + 2 w_bd + 8 w_ss) / N, 16 fp32 ulps of the
largest possible term sum (at most 14 exactly signed terms, the weights' products, their sum).  Gradient,
eps > 0: EPS_GRAD_UNITS of the same scale, four times the largest error measured over the cases below (DESIGN
§11), not below the eps = 0 bound.  Value: 1e-9 relative on grid inputs (every summand exact in fp32, fp64
accumulation), 1e-6 for eps > 0 (the loss tolerance of test_gpu_decoder.py).
"""
import ctypes
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sstv_ref  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 5, 7), (3, 1, 6), (3, 6, 1), (2, 2, 2), (4, 9, 11), (3, 37, 41), (5, 8, 12)]
f32 = lambda v: float(np.float32(v))   # noqa: E731  (the weights as the kernel receives them)
WEIGHTS = {"spatial": (f32(0.05), 0.0, 0.0), "band": (0.0, f32(0.02), 0.0), "sstv": (0.0, 0.0, f32(0.03)),
           "all": (f32(0.05), f32(0.02), f32(0.03))}
EPS = f32(1e-3)
ULP16 = 2.0 ** -20          # 16 fp32 ulps of 1
# eps > 0: the largest gradient error measured on the MI355X over SHAPES x WEIGHTS, in units of
# (4 w_sp + 2 w_bd + 8 w_ss) / N, was 1.9e-6 ((4, 9, 11), SSTV alone; spatial and band alone stay below 1.8e-7).
# It is not the rsqrt: a second difference of fp32 values in [0, 1] carries ~1e-7 of rounding, and phi' has
# slope up to 1 / eps = 1000 where |d| ~ eps, so one term may be off by ~1e-4 of itself (a priori at most ~1e-4
# units over the 8 SSTV terms).  The bound is four times the measured value.
EPS_GRAD_UNITS = max(4 * 1.9e-6, ULP16)


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lrspnp import _lib
    return _lib.device_lib()


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _image(shape, eps):
    if eps == 0.0:
        return sstv_ref.grid_image(shape)
    rng = np.random.default_rng(7 + shape[0] + 31 * shape[1] + 977 * shape[2])
    return rng.random(shape).astype(np.float32)


def _scale(w, n):
    return (4 * w[0] + 2 * w[1] + 8 * w[2]) / n


_REF = {}


def _ref(shape, wname, eps):
    """(R, dR/do) of the case from the fp64 closed form, computed once."""
    key = (shape, wname, eps)
    if key not in _REF:
        _REF[key] = sstv_ref.closed_form(_image(shape, eps).astype(np.float64), *WEIGHTS[wname], eps)
    return _REF[key]


# ---- 1. the kernel alone ------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.0, EPS])
@pytest.mark.parametrize("wname", list(WEIGHTS))
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_vs_fp64(L, shape, wname, eps):
    from lrspnp import ops
    w = WEIGHTS[wname]
    o = _image(shape, eps)
    if eps == 0.0:
        zc = sstv_ref.zero_counts(o)
        assert all((zc[k] > 0) == can for k, can in sstv_ref.kinds_possible(shape).items()), zc
    Rr, gr = _ref(shape, wname, eps)
    val, g = ops.sstv(torch.from_numpy(o).cuda(), spatial=w[0], band=w[1], sstv=w[2], eps=eps)
    torch.cuda.synchronize()
    n = o.size
    err = float(np.abs(g.cpu().numpy().astype(np.float64) - gr).max())
    units = err / _scale(w, n)
    verr = abs(float(val) - Rr)
    print("sstv", shape, wname, eps, "grad err", err, "units", units, "value", float(val), "rel", verr / max(Rr, 1e-300))
    assert units <= (ULP16 if eps == 0.0 else EPS_GRAD_UNITS)
    assert verr <= (1e-9 if eps == 0.0 else 1e-6) * Rr
    if shape == (1, 1, 1):
        assert float(val) == 0.0 and not bool(g.any())


def _framed(o, Hf, Wf, top, left, fill):
    C, H, W = o.shape
    f = torch.full((C, Hf, Wf), fill, dtype=torch.float32)
    f[:, top:top + H, left:left + W] = torch.from_numpy(o)
    return f.cuda()


def _pattern(shape):
    """A known prefill of gout: multiples of 1/8 with both signs."""
    n = int(np.prod(shape))
    return ((torch.arange(n, dtype=torch.float32) % 37) - 18).reshape(shape) / 8


@pytest.mark.parametrize("eps", [0.0, EPS])
def test_accumulates_into_gout_and_loss(L, eps):
    from lrspnp import ops
    w = WEIGHTS["all"]
    o = torch.from_numpy(_image((4, 9, 11), eps)).cuda()
    v0, g0 = ops.sstv(o, spatial=w[0], band=w[1], sstv=w[2], eps=eps)
    pat = _pattern(o.shape).cuda()
    gout = pat.clone()
    acc = torch.full((1,), 3.0, dtype=torch.float64, device="cuda")
    v1, g1 = ops.sstv(o, gout=gout, loss_acc=acc, spatial=w[0], band=w[1], sstv=w[2], eps=eps)
    torch.cuda.synchronize()
    assert g1 is gout and torch.equal(gout, pat + g0)          # one fp32 add per element
    want = 3.0 + float(v0) * o.numel()                          # loss_acc += N R (v0 = N R / N from a zero accumulator)
    assert abs(float(acc) - want) <= 1e-12 * want               # (fp64 atomics from several workgroups, in any order)
    assert abs(float(v1) - float(acc) / o.numel()) <= 1e-15 * float(v1)   # (the device's fp64 division)


@pytest.mark.parametrize("eps", [0.0, EPS])
def test_framed_equals_the_crop(L, eps):
    """C = 3, H x W = 7 x 9 at (2, 3) of a 12 x 16 frame filled with 1e30: the unframed result on the cropped
    image; gout on the frame bit for bit what it was; nothing inf or NaN."""
    from lrspnp import ops
    C, Hf, Wf, top, left, H, W = 3, 12, 16, 2, 3, 7, 9
    w = WEIGHTS["all"]
    o = _image((C, H, W), eps)
    of = _framed(o, Hf, Wf, top, left, 1e30)
    pat = _pattern((C, Hf, Wf)).cuda()
    gf = pat.clone()
    vf, _ = ops.sstv(of, gout=gf, frame=(top, left, H, W), spatial=w[0], band=w[1], sstv=w[2], eps=eps)
    gc = pat[:, top:top + H, left:left + W].contiguous()
    vc, _ = ops.sstv(torch.from_numpy(o).cuda(), gout=gc, spatial=w[0], band=w[1], sstv=w[2], eps=eps)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(gf).all()) and np.isfinite(float(vf))
    assert torch.equal(gf[:, top:top + H, left:left + W], gc)
    inside = torch.zeros((Hf, Wf), dtype=torch.bool, device="cuda")
    inside[top:top + H, left:left + W] = True
    assert torch.equal(gf[:, ~inside], pat[:, ~inside])
    assert abs(float(vf) - float(vc)) <= 1e-12 * float(vc)       # the same summands; fp64 atomics in any order
    Rr, gr = sstv_ref.closed_form(o.astype(np.float64), *w, eps)
    err = float(np.abs((gf - pat)[:, top:top + H, left:left + W].cpu().numpy().astype(np.float64) - gr).max())
    assert err <= EPS_GRAD_UNITS * _scale(w, o.size) + 2.0 ** -23 * float(pat.abs().max())   # + the add's rounding


@pytest.mark.parametrize("eps", [0.0, EPS])
@pytest.mark.parametrize("shape", [(5, 8, 12), (3, 7, 9)])
def test_deterministic_and_float4_equals_scalar(L, shape, eps):
    """Two runs give the same bits; the same image at an aligned left (float4 loads and stores; W = 9: a
    partial last strip whose 16-byte load reaches into the 1e30 frame) and at a misaligned one (scalar form),
    and unframed, give the same bits."""
    from lrspnp import ops
    C, H, W = shape
    w = WEIGHTS["all"]
    o = _image(shape, eps)
    kw = dict(spatial=w[0], band=w[1], sstv=w[2], eps=eps)
    res = []
    for left, Wf in ((4, 20), (3, 20), (4, 20), (1, 19)):
        of = _framed(o, H + 3, Wf, 2, left, 1e30)
        _, g = ops.sstv(of, frame=(2, left, H, W), **kw)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(g).all())
        res.append(g[:, 2:2 + H, left:left + W].clone())
    _, g = ops.sstv(torch.from_numpy(o).cuda(), **kw)
    torch.cuda.synchronize()
    for r in res:
        assert torch.equal(r, g)
    assert float(g.abs().max()) > 0


def test_refusals(L):
    o = torch.zeros((3, 12, 16), device="cuda")
    pat = _pattern((3, 12, 16)).cuda()
    g = pat.clone()
    acc = torch.zeros(1, dtype=torch.float64, device="cuda")
    ok = dict(C=3, Hf=12, Wf=16, top=2, left=3, H=7, W=9, sp=0.05, bd=0.02, ss=0.03, eps=1e-3, n=3 * 7 * 9)

    def call(out=o, **kw):
        a = dict(ok, **kw)
        return L.lrs_sstv_f32(P(out), a["C"], a["Hf"], a["Wf"], a["top"], a["left"], a["H"], a["W"], a["sp"], a["bd"],
                              a["ss"], a["eps"], a["n"], P(g), P(acc), S())

    assert call(out=None) == -1
    for k in ("C", "Hf", "Wf", "H", "W"):
        assert call(**{k: 0}) == -1 and call(**{k: -2}) == -1, k
    assert call(top=-1) == -1 and call(left=-1) == -1
    assert call(top=6) == -1 and call(left=8) == -1 and call(H=13) == -1 and call(W=17) == -1
    for k in ("sp", "bd", "ss", "eps"):
        assert call(**{k: -1e-3}) == -1, k
    assert call(n=0) == -1
    assert call(sp=0.0, bd=0.0, ss=0.0) == 0      # all weights 0: nothing launched
    torch.cuda.synchronize()
    assert torch.equal(g, pat) and float(acc) == 0.0
    assert call() == 0                             # (the arguments above were otherwise valid)
    torch.cuda.synchronize()
    # a constant image: every derivative term is 0, every phi is eps
    assert torch.equal(g, pat)
    want = 1e-3 * (0.05 * 3 * (6 * 9 + 7 * 8) + 0.02 * 2 * 7 * 9 + 0.03 * 2 * (6 * 9 + 7 * 8))   # N R
    assert abs(float(acc) - want) <= 1e-6 * want

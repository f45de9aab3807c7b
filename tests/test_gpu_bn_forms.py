"""GPU: every form of the DIP BatchNorm family (csrc/dip_bn.h) that the primitive ABI reaches, through
lrs_bn_act_fwd_f32 / lrs_bn_act_bwd_f32 alone, against fp64 torch on the CPU.

The form is picked from P (bn_split, bn_one_wg, bn_reg_q, bn1_threads); torch allocations are 16-byte
aligned, so P % 4 decides the float4 path.  The construction is test_bn_act's (test_gpu_dip.py): gamma
with max > 1 so that the Lipschitz rescale is active, running statistics checked, the conv-bias gradient
held to its noise scale; the tolerances are that test's, the same kernels and arithmetic:
y 1e-5, gz / ggamma / gbeta 2e-5, running statistics 1e-5, |gbias - sum gz| <= 1e-5 sum|gz| + 1e-6.

The forms only the engine launches (k_reduce_bn1, k_bn_fwd_r on split-K partials or with the raw-weight
scale, k_reduce_bn_bwd1, accum, k_conv_bn_dir) stay with test_gpu_dip.py's whole-net tests.
tools/bn_forms_digest.py hashes the outputs of the same cases (run_case) for bitwise comparisons.
"""
import ctypes

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

LRELU, SIGMOID, NONE = 1, 2, 0

# (C, P, act)
CASES = [
    # k_bn_fwd1 / k_bn_bwd1 on 256 threads
    (5, 1, LRELU),         # one-pixel channel: the P > 1 guard of the unbiased variance
    (5, 100, SIGMOID),     # bn_needs_y: the backward reads y
    (5, 512, LRELU),       # last P on 256 threads (kBn1SmallMaxP)
    # ... on 1,024 threads
    (5, 513, LRELU),       # first P on 1,024 threads, scalar path
    (5, 513, NONE),        # no activation
    (70, 513, LRELU),      # bn_lip_scale_w loops over more than 64 channels
    (5, 4095, LRELU),      # scalar path
    (5, 4096, LRELU),      # last P of the one-workgroup form, float4 path
    # k_bn_fwd_r / k_bn_bwd_r
    (5, 4100, LRELU),      # nq 2, second quad row almost empty
    (5, 4100, SIGMOID),
    (70, 4100, LRELU),     # more than 64 channels
    (5, 8192, LRELU),      # nq 2, second quad row full
    (5, 8196, LRELU),      # first P of nq 3
    (5, 12292, LRELU),     # first P of nq 4
    (5, 16388, LRELU),     # bn_reg_q rounds q = 5 up to 6
    (5, 24580, LRELU),     # bn_reg_q rounds q = 7 up to 8
    (5, 32772, LRELU),     # first P of nq 10
    (5, 40960, LRELU),     # last P of the register form
    # S-way split with BN
    (5, 4099, LRELU),      # scalar, S = 2, ragged chunk
    (5, 4099, SIGMOID),
    (70, 4099, LRELU),     # bn_lip_scale (whole block) over more than 64 channels
    (5, 40964, LRELU),     # float4: first P past the register form; chunk rounded to 4
    (2, 262148, LRELU),    # S capped at 64
]


def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-300))


def inputs(C, HW):
    g = torch.Generator().manual_seed(C + HW)
    z = torch.randn(C, HW, generator=g) * 2 + 0.5
    gamma = 1 + 0.5 * torch.rand(C, generator=g)       # max > 1: the Lipschitz rescale is active
    beta = 0.2 * torch.randn(C, generator=g)
    gy = torch.randn(C, HW, generator=g)
    return z, gamma, beta, gy


def run_case(L, C, HW, act):
    """The library's outputs of one case, as a dict of device tensors (and the inputs, on the CPU)."""
    z, gamma, beta, gy = inputs(C, HW)
    zd, gmd, btd, gyd = (t.cuda().contiguous() for t in (z, gamma, beta, gy))
    o = {k: torch.empty_like(zd) for k in ("y", "gz")}
    for k in ("mean", "invstd", "ggamma", "gbeta", "gbias"):
        o[k] = torch.empty(C, device="cuda")
    o["run_mean"], o["run_var"] = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    nws = L.lrs_bn_act_workspace(C, HW)
    ws = torch.zeros(nws, dtype=torch.uint8, device="cuda")
    assert L.lrs_bn_act_fwd_f32(_P(zd), _P(o["y"]), _P(gmd), _P(btd), _P(o["mean"]), _P(o["invstd"]), _P(o["run_mean"]),
                                _P(o["run_var"]), C, HW, act, ctypes.c_float(1e-5), ctypes.c_float(0.1), _P(ws), nws,
                                _S()) == 0
    assert L.lrs_bn_act_bwd_f32(_P(gyd), _P(o["y"]), _P(zd), _P(gmd), _P(o["mean"]), _P(o["invstd"]), _P(o["gz"]),
                                _P(o["ggamma"]), _P(o["gbeta"]), _P(o["gbias"]), C, HW, act, _P(ws), nws, _S()) == 0
    torch.cuda.synchronize()
    return o, (z, gamma, beta, gy)


def reference(z, gamma, beta, gy, act):
    """fp64: BatchNorm2d in train mode (biased variance, eps 1e-5) on gamma / c, beta / c with
    c = max(max|gamma|, 1) held constant, then the activation; its gradients; the running statistics."""
    zr, gr, br = (t.double().clone().requires_grad_(True) for t in (z, gamma, beta))
    c = max(float(gamma.double().abs().max()), 1.0)
    m, var = zr.mean(1, keepdim=True), zr.var(1, unbiased=False, keepdim=True)
    h = (zr - m) / torch.sqrt(var + 1e-5) * (gr / c)[:, None] + (br / c)[:, None]
    yr = torch.nn.functional.leaky_relu(h, 0.2) if act == LRELU else torch.sigmoid(h) if act == SIGMOID else h
    yr.backward(gy.double())
    HW = z.shape[1]
    unb = var.detach()[:, 0] * (HW / (HW - 1) if HW > 1 else 1.0)   # P == 1: the biased variance (0) stands in
    return {"y": yr.detach(), "gz": zr.grad, "ggamma": gr.grad, "gbeta": br.grad,
            "run_mean": 0.1 * m.detach()[:, 0], "run_var": 0.9 + 0.1 * unb}


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lrspnp import _lib
    return _lib.device_lib()


@pytest.mark.parametrize("C,HW,act", CASES)
def test_bn_form(L, C, HW, act):
    o, (z, gamma, beta, gy) = run_case(L, C, HW, act)
    r = reference(z, gamma, beta, gy, act)
    err = {k: _rel(o[k], r[k]) for k in ("y", "gz", "ggamma", "gbeta", "run_mean", "run_var")}
    gsum, gabs = r["gz"].sum(1), r["gz"].abs().sum(1)
    gb = o["gbias"].cpu().double() - gsum
    gb_ratio = float((gb.abs() / (1e-5 * gabs + 1e-6)).max())   # <= 1: within the noise scale
    print(f"bn_form C={C} P={HW} act={act}: " + " ".join(f"{k}={v:.3e}" for k, v in err.items())
          + f" gbias/noise={gb_ratio:.3e}")
    assert err["y"] < 1e-5
    assert err["gz"] < 2e-5
    # conv-bias grad = sum_p gz: ~0 under a BN (rounding noise), so held to the noise scale
    assert gb_ratio <= 1.0
    assert err["ggamma"] < 2e-5 and err["gbeta"] < 2e-5
    assert err["run_var"] < 1e-5 and err["run_mean"] < 1e-5

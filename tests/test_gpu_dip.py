"""GPU: DIP low-rank prox kernels (lrs_conv2d_*, lrs_bn_act_*, lrs_sigma_max_f32, lrs_adam_f32,
lrs_masked_mse_f32, lrs_es_*) and the lrs_dipnet engine, against plain PyTorch fp32 on the CPU
(tests/dip_ref.py, itself pinned to the reference's my_Lipschitz_Unet by tests/test_dip_ref.py).

Tolerances (relative L2 unless noted): single layers 1e-5 (fwd) / 2e-5 (bwd); sigma_max 2e-6
vs fp64 SVD; whole-net forward 1e-5, loss 1e-6, step-0 gradients 1e-4; Adam 1e-6.
Multi-step trajectories are chaotic (see test_dip_ref.py) and are compared step by step from
identical states instead.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import dip_ref  # noqa: E402
from lrspnp import _lib  # noqa: E402

pytestmark = pytest.mark.gpu


def rel(a, b):
    a = torch.as_tensor(a).double().cpu(); b = torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-300))


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


CONV_CASES = [
    # cin, cout, H, W, k, stride, pad, pad_mode, up
    (128, 128, 36, 36, 3, 2, 1, 1, 0),      # d_1 first conv
    (128, 128, 18, 18, 3, 1, 1, 1, 0),
    (128, 128, 3, 3, 3, 1, 1, 1, 0),        # bottleneck: reflection on a 3x3 map (3 mirrors)
    (128, 128, 3, 3, 2, 1, 0, 1, 1),        # up_1: upsample + 2x2
    (128, 128, 9, 9, 3, 1, 1, 1, 1),        # up_3
    (128, 198, 36, 36, 1, 1, 0, 1, 0),      # last 1x1 (plain)
    (7, 5, 11, 6, 3, 2, 1, 0, 0),           # zero padding, odd sizes
    (5, 9, 5, 7, 3, 1, 1, 1, 1),
    (128, 128, 196, 196, 3, 1, 1, 1, 0),    # 196x196 layer: 128x128 GEMM tiles (split-bf16 path)
    (64, 96, 100, 90, 3, 2, 1, 0, 0),       # 128-tiles with ragged M, N and K
    (128, 198, 196, 196, 1, 1, 0, 1, 0),    # 196x196 last 1x1 (k_pw with col == NULL: 4 row blocks)
    (198, 128, 40, 41, 1, 1, 0, 1, 0),      # k_pw: K = 198 (planes padded to 208), N % 64 != 0
    (37, 250, 9, 13, 1, 1, 0, 1, 0),        # k_pw: ragged K, M = 250
    (128, 128, 49, 49, 3, 1, 1, 1, 1),      # up_3 at 196x196: effective 4x4 stride-2 data gradient + reflection border
    (64, 32, 10, 7, 3, 1, 1, 0, 1),         # upsampled zero-padded 3x3: effective kernel, no border terms
    (128, 128, 25, 25, 2, 1, 0, 1, 1),      # up_2: effective 3x3 stride-2 data gradient
    (24, 40, 2, 5, 3, 1, 1, 1, 1),          # reflection border on a 2-row source (corners only)
    (198, 128, 200, 200, 1, 1, 0, 1, 0),    # k_pw, K = 198 over 40,000 pixels: B staged in chunks (128 + 96)
    (160, 48, 150, 150, 1, 1, 0, 1, 0),     # k_pw, K = 160 in chunks (128 + 32: a partial k-step chunk)
]


def torch_conv(x, w, b, k, stride, pad, pad_mode, up):
    h = x[None]
    if up:
        h = F.interpolate(h, scale_factor=2, mode="nearest")
    if pad:
        h = F.pad(h, (pad,) * 4, mode="reflect" if pad_mode == 1 else "constant")
    return F.conv2d(h, w, b, stride=stride)[0]


@pytest.fixture(params=["split_bf16", "f32"])
def precision(request, L):
    # lrs_dip_opts.precision per call: LRS_DIP_SPLIT_BF16 = 1 (default), LRS_DIP_F32 = 0
    return ctypes.byref(_lib.dip_opts(1 if request.param == "split_bf16" else 0))


def test_dip_opts_rejects_bad_precision(L):
    o = _lib.dip_opts(7)
    assert L.lrs_conv2d_workspace(8, 8, 8, 8, 3, 1, 1, 0, ctypes.byref(o)) == 0
    x = torch.zeros(8, 8, 8, device="cuda")
    assert L.lrs_conv2d_fwd_f32(P(x), 8, 8, 8, P(x), None, 8, 3, 1, 1, 1, 0, None, P(x), ctypes.byref(o),
                                None, 0, S()) == -1


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_fwd_bwd(L, case, precision):
    cin, cout, H, W, k, stride, pad, pm, up = case
    g = torch.Generator().manual_seed(hash(case) & 0xffff)
    x = torch.randn(cin, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / np.sqrt(cin * k * k)
    b = torch.randn(cout, generator=g) * 0.1
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    yr = torch_conv(xr, wr, b, k, stride, pad, pm, up)
    gy = torch.randn(yr.shape, generator=g)
    yr.backward(gy)
    Ho, Wo = yr.shape[1:]
    xd, wd, bd, gyd = (t.cuda().contiguous() for t in (x, w, b, gy))
    ncol = L.lrs_conv2d_col_size(cin, H, W, k, stride, pad, up)
    col = torch.empty(max(ncol, 1), device="cuda")
    nws = L.lrs_conv2d_workspace(cin, H, W, cout, k, stride, pad, up, precision)
    ws = torch.empty(nws // 4 + 1, device="cuda")
    y = torch.empty(cout, Ho, Wo, device="cuda")
    assert L.lrs_conv2d_fwd_f32(P(xd), cin, H, W, P(wd), P(bd), cout, k, stride, pad, pm, up,
                                P(col) if ncol else None, P(y), precision, P(ws), nws, S()) == 0
    assert rel(y, yr.detach()) < 1e-5
    div = torch.tensor([1.7], device="cuda")
    gw = torch.empty_like(wd)
    gx = torch.empty_like(xd)
    assert L.lrs_conv2d_bwd_f32(P(gyd), P(col) if ncol else P(xd), P(wd), P(div), cin, H, W, cout, k, stride,
                                pad, pm, up, P(gx), P(gw), precision, P(ws), nws, S()) == 0
    torch.cuda.synchronize()
    assert rel(gw, wr.grad / 1.7) < 2e-5
    assert rel(gx, xr.grad) < 2e-5


@pytest.fixture(params=[0, 1], ids=["fold", "upeff"])
def upsample_dgrad(L, request):
    # lrs_dip_opts.upsample_dgrad, per call / per net
    return request.param


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_implicit_fwd_bwd(L, case, upsample_dgrad):
    # col == NULL: the split-bf16 implicit-GEMM conv (im2col gathered in the kernel), and
    # lrs_conv2d_bwd_x_f32 (dW's col^T gathered from x); same tolerances as the explicit path
    cin, cout, H, W, k, stride, pad, pm, up = case
    g = torch.Generator().manual_seed(hash(case) & 0xffff)
    x = torch.randn(cin, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / np.sqrt(cin * k * k)
    b = torch.randn(cout, generator=g) * 0.1
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    yr = torch_conv(xr, wr, b, k, stride, pad, pm, up)
    gy = torch.randn(yr.shape, generator=g)
    yr.backward(gy)
    xd, wd, bd, gyd = (t.cuda().contiguous() for t in (x, w, b, gy))
    opts = ctypes.byref(_lib.dip_opts(1, upsample_dgrad))
    nws = L.lrs_conv2d_workspace(cin, H, W, cout, k, stride, pad, up, opts)
    ws = torch.empty(nws // 4 + 1, device="cuda")
    y = torch.full(yr.shape, float("nan"), device="cuda")
    assert L.lrs_conv2d_fwd_f32(P(xd), cin, H, W, P(wd), P(bd), cout, k, stride, pad, pm, up,
                                None, P(y), opts, P(ws), nws, S()) == 0
    assert rel(y, yr.detach()) < 1e-5
    div = torch.tensor([1.7], device="cuda")
    gw = torch.full_like(wd, float("nan"))
    gx = torch.full_like(xd, float("nan"))
    assert L.lrs_conv2d_bwd_x_f32(P(gyd), P(xd), P(wd), P(div), cin, H, W, cout, k, stride,
                                  pad, pm, up, P(gx), P(gw), opts, P(ws), nws, S()) == 0
    torch.cuda.synchronize()
    assert rel(gw, wr.grad / 1.7) < 2e-5
    assert rel(gx, xr.grad) < 2e-5


@pytest.mark.parametrize("bn,act,C,HW", [(1, 1, 128, 36 * 36), (1, 1, 64, 9), (0, 1, 198, 1296), (1, 2, 16, 100),
                                         (1, 1, 128, 196 * 196), (0, 1, 8, 50000)])
def test_bn_act(L, bn, act, C, HW):
    g = torch.Generator().manual_seed(C + HW)
    z = torch.randn(C, HW, generator=g) * 2 + 0.5
    gamma = 1 + 0.5 * torch.rand(C, generator=g)       # max > 1: the Lipschitz rescale is active
    beta = 0.2 * torch.randn(C, generator=g)
    gy = torch.randn(C, HW, generator=g)
    zr, gr, br = z.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    h = zr[None, :, :, None]
    if bn:
        c = max(float(gamma.abs().max()), 1.0)
        h = F.batch_norm(h, None, None, gr / c, br / c, training=True, eps=1e-5)
    yr = (F.leaky_relu(h, 0.2) if act == 1 else torch.sigmoid(h))[0, :, :, 0]
    yr.backward(gy)
    zd, gmd, btd, gyd = (t.cuda().contiguous() for t in (z, gamma, beta, gy))
    y = torch.empty_like(zd)
    mean, istd = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    nws = L.lrs_bn_act_workspace(C, HW)
    ws = torch.zeros(nws, dtype=torch.uint8, device="cuda")
    assert L.lrs_bn_act_fwd_f32(P(zd), P(y), P(gmd) if bn else None, P(btd) if bn else None, P(mean), P(istd),
                                P(rm) if bn else None, P(rv) if bn else None, C, HW, act, ctypes.c_float(1e-5),
                                ctypes.c_float(0.1), P(ws), nws, S()) == 0
    assert rel(y, yr.detach()) < 1e-5
    gz = torch.empty_like(zd)
    gg, gb, gbias = torch.empty(C, device="cuda"), torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    assert L.lrs_bn_act_bwd_f32(P(gyd), P(y), P(zd), P(gmd) if bn else None, P(mean), P(istd), P(gz),
                                P(gg) if bn else None, P(gb) if bn else None, P(gbias), C, HW, act, P(ws), nws,
                                S()) == 0
    torch.cuda.synchronize()
    assert rel(gz, zr.grad) < 2e-5
    # conv-bias grad = sum_p gz: ~0 under a BN (rounding noise), so held to the noise scale
    gsum, gabs = zr.grad.double().sum(1), zr.grad.double().abs().sum(1)
    assert bool(((gbias.cpu().double() - gsum).abs() <= 1e-5 * gabs + 1e-6).all())
    if bn:
        assert rel(gg, gr.grad) < 2e-5 and rel(gb, br.grad) < 2e-5
        var = z.double().var(1, unbiased=True)
        assert rel(rv, 0.9 + 0.1 * var) < 1e-5 and rel(rm, 0.1 * z.double().mean(1)) < 1e-5


# k_conv_bn_dir (dip_dir.h) through lrs_conv_bn_small_f32: every branch dir_geom admits.
# cin, cout, H, W, k, stride, bias, lip, act
CONV_BN_DIR_CASES = [
    (128, 128, 9, 9, 3, 1, True, 1, 1),      # U-Net 9^2 layer: scalar staging (81 % 4 != 0), one chunk
    (128, 128, 18, 18, 3, 2, True, 1, 1),    # 18^2 -> 9^2: 16-B staging, two chunks (101 + 27 channels)
    (256, 64, 9, 9, 3, 1, True, 1, 1),       # scalar staging, two chunks (202 + 54)
    (128, 128, 5, 5, 3, 1, False, 0, 0),     # no bias, plain BatchNorm, no activation
    (128, 96, 9, 9, 3, 2, True, 0, 1),       # 9^2 -> 5^2, stride 2, scalar staging
    (200, 16, 3, 3, 3, 1, True, 1, 1),       # 3^2 map: the reflection reaches across the whole map
    (32, 24, 2, 2, 3, 1, True, 1, 2),        # 2^2 source (the smallest a reflection admits), sigmoid
    (64, 32, 8, 8, 1, 1, True, 1, 2),        # 1x1, 16-B staging
    (48, 40, 10, 10, 1, 2, False, 1, 1),     # 1x1 stride 2, 10^2 -> 5^2
    (16, 8, 24, 12, 3, 2, True, 1, 1),       # non-square, 12 x 6 output
    (7, 5, 6, 7, 3, 1, True, 1, 1),          # ragged channels, a row of 7 (two strips, one partial)
]


def _conv_bn_ref(x, w, b, gamma, beta, k, stride, lip, act):
    """fp64 Conv2d(ReflectionPad) -> BatchNorm2d(train) [/ BatchNormSpectralNorm] -> act."""
    h = x.double()[None]
    if k == 3:
        h = F.pad(h, (1, 1, 1, 1), mode="reflect")
    z = F.conv2d(h, w.double(), None if b is None else b.double(), stride=stride)
    c = max(float(gamma.abs().max()), 1.0) if lip else 1.0
    zm = z.mean((0, 2, 3))
    var = z.var((0, 2, 3), unbiased=False)
    yb = (z - zm[None, :, None, None]) / torch.sqrt(var + 1e-5)[None, :, None, None]
    yb = yb * (gamma.double() / c)[None, :, None, None] + (beta.double() / c)[None, :, None, None]
    y = F.leaky_relu(yb, 0.2) if act == 1 else torch.sigmoid(yb) if act == 2 else yb
    P = z.shape[2] * z.shape[3]
    return z[0], y[0], zm, 1.0 / torch.sqrt(var + 1e-5), var * P / max(P - 1, 1)


@pytest.mark.parametrize("case", CONV_BN_DIR_CASES)
def test_conv_bn_small_one_launch(L, case):
    cin, cout, H, W, k, stride, has_bias, lip, act = case
    g = torch.Generator().manual_seed(cin * 131 + cout * 7 + H + k + stride)
    x = torch.randn(cin, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / np.sqrt(cin * k * k)
    b = torch.randn(cout, generator=g) * 0.1 if has_bias else None
    gamma = 0.6 + 0.9 * torch.rand(cout, generator=g)     # max > 1: the Lipschitz rescale acts
    beta = 0.2 * torch.randn(cout, generator=g)
    zr, yr, mr, isr, vr = _conv_bn_ref(x, w, b, gamma, beta, k, stride, lip, act)
    xd, wd, gd, btd = (t.cuda().contiguous() for t in (x, w, gamma, beta))
    bd = b.cuda() if has_bias else None
    z = torch.full(zr.shape, float("nan"), device="cuda")
    y = torch.full(zr.shape, float("nan"), device="cuda")
    mean, istd = torch.full((cout,), float("nan"), device="cuda"), torch.full((cout,), float("nan"), device="cuda")
    rm, rv = 0.3 * torch.ones(cout, device="cuda"), 2.0 * torch.ones(cout, device="cuda")
    rc = L.lrs_conv_bn_small_f32(P(xd), cin, H, W, P(wd), P(bd), cout, k, stride, (k - 1) // 2, 1, 0, P(gd), P(btd),
                                 lip, act, P(z), P(y), P(mean), P(istd), P(rm), P(rv), S())
    assert rc == 0
    torch.cuda.synchronize()
    assert rel(z, zr) < 1e-5
    assert rel(y, yr) < 1e-5
    assert rel(mean, mr) < 1e-5
    assert rel(istd, isr) < 1e-5
    assert rel(rm, 0.9 * 0.3 + 0.1 * mr) < 1e-5
    assert rel(rv, 0.9 * 2.0 + 0.1 * vr) < 1e-5
    # without running statistics: the same outputs, bit for bit
    z2, y2 = torch.empty_like(z), torch.empty_like(y)
    m2, i2 = torch.empty_like(mean), torch.empty_like(istd)
    assert L.lrs_conv_bn_small_f32(P(xd), cin, H, W, P(wd), P(bd), cout, k, stride, (k - 1) // 2, 1, 0, P(gd),
                                   P(btd), lip, act, P(z2), P(y2), P(m2), P(i2), None, None, S()) == 0
    torch.cuda.synchronize()
    assert torch.equal(z2, z) and torch.equal(y2, y) and torch.equal(m2, mean) and torch.equal(i2, istd)


@pytest.mark.parametrize("cin,H,W,k,stride,pad,pm,up,why", [
    (16, 9, 9, 3, 1, 1, 0, 0, "zero padding"),
    (16, 5, 5, 3, 1, 1, 1, 1, "upsample"),
    (16, 1, 6, 1, 1, 0, 1, 0, "a one-row source"),
    (8, 40, 40, 1, 1, 0, 1, 0, "1600 output pixels"),
    (16, 30, 30, 3, 1, 1, 1, 0, "150 row strips (over 64)"),
    (400, 18, 18, 3, 2, 1, 1, 0, "four staged chunks"),
    (16, 9, 9, 2, 1, 0, 1, 0, "a 2 x 2 kernel"),
])
def test_conv_bn_small_refuses(L, cin, H, W, k, stride, pad, pm, up, why):
    t = torch.zeros(max(cin * 4 * H * W * 9, 64), device="cuda")
    c = torch.ones(8, device="cuda")
    assert L.lrs_conv_bn_small_f32(P(t), cin, H, W, P(t), None, 8, k, stride, pad, pm, up, P(c), P(c), 1, 1,
                                   P(t), P(t), P(c), P(c), None, None, S()) == -2, why


def test_sigma_max(L):
    from lrspnp.dip import sigma_max
    g = torch.Generator().manual_seed(5)
    mats = [torch.randn(128, 1152, generator=g) * 0.04, torch.randn(128, 512, generator=g) * 0.06,
            torch.randn(128, 128, generator=g) * 0.1, torch.randn(198, 128, generator=g) * 0.1,
            torch.randn(7, 3, generator=g),
            (torch.randn(128, 4, generator=g) @ torch.randn(4, 300, generator=g)) * 0.01,   # rank 4
            torch.full((64, 64), 0.01)]                                                    # rank 1
    sig, sc = sigma_max([m.cuda() for m in mats])
    ref = torch.tensor([float(torch.linalg.svdvals(m.double())[0]) for m in mats])
    np.testing.assert_allclose(sig.cpu().double().numpy(), ref.numpy(), rtol=2e-6)
    # within one float32 ulp of the fp64 SVD value (the guarantee and its exception: tests/test_gpu_sigma.py)
    r32 = ref.numpy().astype(np.float32)
    assert (np.abs(sig.cpu().numpy() - r32) <= np.spacing(r32)).all(), (sig.cpu().numpy() - r32) / np.spacing(r32)
    np.testing.assert_allclose(sc.cpu().numpy(), np.maximum(1.0, sig.cpu().numpy()))


def test_adam_matches_torch(L):
    g = torch.Generator().manual_seed(2)
    p0 = torch.randn(10007, generator=g)
    p = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=0.1)
    pd, md, vd = p0.cuda(), torch.zeros(10007, device="cuda"), torch.zeros(10007, device="cuda")
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    for it in range(4):
        gr = torch.randn(10007, generator=g) * (10.0 ** -it)
        p.grad = gr.clone()
        opt.step()
        step += 1
        assert L.lrs_adam_f32(P(pd), P(gr.cuda()), P(md), P(vd), 10007, P(step), ctypes.c_float(0.1),
                              ctypes.c_float(0.9), ctypes.c_float(0.999), ctypes.c_float(1e-8), S()) == 0
        torch.cuda.synchronize()
        assert rel(pd, p.detach()) < 1e-6


@pytest.mark.parametrize("C,H,W", [(128, 36, 36), (7, 35, 37), (198, 196, 196)])
def test_masked_mse(L, C, H, W):
    """Both kernel paths: float4 (H*W % 4 == 0) and scalar (35x37), one to many workgroups per channel."""
    g = torch.Generator().manual_seed(3)
    out, tgt = torch.randn(C, H, W, generator=g), torch.randn(C, H, W, generator=g)
    mask = (torch.rand(H, W, generator=g) > 0.3).float()
    o = out.clone().requires_grad_(True)
    loss = F.mse_loss(tgt * mask, o * mask)
    loss.backward()
    acc = torch.zeros(1, dtype=torch.float64, device="cuda")
    gout = torch.empty(C, H, W, device="cuda")
    assert L.lrs_masked_mse_f32(P(out.cuda()), P(tgt.cuda()), P(mask.cuda()), C, H * W, P(gout), P(acc), S()) == 0
    torch.cuda.synchronize()
    assert abs(float(acc) / out.numel() - float(loss.detach())) < 1e-6 * float(loss.detach())
    assert rel(gout, o.grad) < 1e-6


def test_early_stop_device_vs_reference_logic(L):
    from lrspnp.dip import EarlyStopper
    g = torch.Generator().manual_seed(4)
    N, size, patience = 500, 5, 4
    es = EarlyStopper(N, size, patience)
    ref = dip_ref.EarlyStopRef(size, patience)
    base = torch.randn(N, generator=g)
    stop_ref = None
    for i in range(40):
        scale = 1.0 / (1 + i) if i < 12 else 0.05 * (1 + (i % 3))   # variance falls, then plateaus
        img = base + scale * torch.randn(N, generator=g)
        if ref.update(img.numpy(), i) and stop_ref is None:
            stop_ref = ref.stop_epoch
        assert L.lrs_es_update_f32(P(img.cuda()), N, P(es.ring), P(es.state), None) == 0
    st = es.read()
    assert stop_ref is not None and st.stop == 1 and st.stop_epoch == stop_ref
    np.testing.assert_allclose(st.best, min(ref.vars), rtol=1e-9)


def test_stream_wait_orders_streams(L):
    """lrs_stream_wait (dip.stream_wait, the DIP stream's ordering against the caller's): work enqueued
    on the waiter after the call sees the signaller's earlier writes, even behind a long kernel."""
    from lrspnp.dip import stream_wait
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    x = torch.zeros(1 << 22, device="cuda")
    for v in (3.0, 5.0):
        with torch.cuda.stream(a):
            torch.cuda._sleep(20_000_000)      # ~10 ms of spinning before the write
            x.fill_(v)
        stream_wait(b, a)
        with torch.cuda.stream(b):
            y = x * 2.0
        b.synchronize()
        assert bool((y == 2.0 * v).all())
    torch.cuda.synchronize()


def test_early_stop_sliding_sums_over_many_windows(L):
    """The ES window sums slide from step to step and are re-summed from the ring every 10 windows
    (k_es_step / k_es_decide): over 700 updates -- two re-sums, the fill, the wrap -- every variance
    the device forms matches the last 30 outputs' variance recomputed in fp64 to 1e-10."""
    from lrspnp.dip import EarlyStopper
    g = torch.Generator().manual_seed(11)
    N, size = 3001, 30
    es = EarlyStopper(N, size, 10 ** 6)
    base = torch.rand(N, generator=g, dtype=torch.float64) * 0.8
    hist = []
    for i in range(700):
        img = (base + (0.05 + 0.04 * np.sin(i / 17.0)) * torch.randn(N, generator=g, dtype=torch.float64)).float()
        hist.append(img.double())
        assert L.lrs_es_update_f32(P(img.cuda()), N, P(es.ring), P(es.state), None) == 0
        if i + 1 >= size and (i % 37 == 0 or i in (size - 1, 299, 300, 599, 600, 699)):
            st = es.read()
            w = torch.stack(hist[-size:])
            ref = float(((w - w.mean(0)) ** 2).sum()) / N / size
            assert abs(st.last_var - ref) <= 1e-10 * ref, (i, st.last_var, ref)
    assert es.read().count == 700


def test_early_stop_device_vs_reference_golden(L, golden):
    """lrs_es_update_f32 against the reference's own get_DIP_out early stopping (EarlyStop +
    myMetric, float32 numpy; tests/golden/gen_es_golden.py) on three recorded trajectories: the
    device stops at the step where the reference returned (or never), its best variance matches
    the reference's best_score to 1e-5 relative (fp64 vs float32 sums), and every variance it
    computed (last_var) matches the reference's cur_var to 1e-5."""
    from lrspnp.dip import EarlyStopper
    g = golden("es_golden.npz")
    for k in range(3):
        traj = torch.from_numpy(g[f"traj{k}"]).cuda()
        T, N = traj.shape[0], traj[0].numel()
        es = EarlyStopper(N, int(g["size"]), int(g["patience"]))
        ref_var = dict(zip(g[f"epoch{k}"].tolist(), g[f"var{k}"].tolist()))
        stop_at = -1
        for i in range(T):
            assert L.lrs_es_update_f32(P(traj[i]), N, P(es.ring), P(es.state), None) == 0
            st = es.read()
            if i in ref_var:
                assert abs(st.last_var - ref_var[i]) <= 1e-5 * ref_var[i], (k, i)
            if st.stop and stop_at < 0:
                stop_at = i
                assert st.stop_epoch == i
                break
        assert stop_at == int(g[f"ret{k}"]), (k, stop_at)
        assert abs(st.best - float(g[f"best{k}"])) <= 1e-5 * float(g[f"best{k}"])
        assert st.best_epoch == int(g[f"best_epoch{k}"])


# ---- whole network -----------------------------------------------------------------------------
def _problem(gold_seed=1234, units=None):
    from gen_dip_golden import flat_params, problem
    from lrspnp.dip import lipschitz_unet_units
    units = units or lipschitz_unet_units(128, 128, 128)
    flat = torch.from_numpy(flat_params(units, gold_seed))
    x, t, m = (torch.from_numpy(a) for a in problem(gold_seed))
    return units, flat, x, t, m


def _engine(units, flat, H=36, W=36, C=128, **opts):
    from lrspnp.dip import DipNet
    net = DipNet(units, C, H, W, **opts)
    net.params.copy_(flat.cuda())
    net.reset_optimizer()
    return net


def test_unet_forward_and_first_step_vs_reference(L, golden):
    gold = golden("dip_golden.npz")
    units, flat, x, t, m = _problem(int(gold["seed"]))
    net = _engine(units, flat)
    out = net.forward(x.cuda()).cpu()
    sub = int(gold["sub"])
    assert rel(out.reshape(-1)[::sub], torch.from_numpy(gold["out_sub"][0])) < 1e-5     # the reference module
    ref = dip_ref.forward(flat, units, x)
    assert rel(out, ref) < 1e-5
    # one training step from the same state: loss, gradients, the Adam update.  Gradients are
    # compared with the restatement in fp64 (the engine is ~2e-5 from it; fp32 CPU torch on the GPU
    # hosts measured 1.8e-3 from fp64 at the first layer, so fp32 CPU is not a tight reference).
    tr = dip_ref.RefTrainer(units, flat)
    out_r, loss_r, _ = tr.step(x, t, m.reshape(-1))
    p64 = flat.double().clone().requires_grad_(True)
    dip_ref.loss_fn(dip_ref.forward(p64, units, x.double()), t.double(), m.reshape(-1).double()).backward()
    g_r = p64.grad
    net.train_steps(x.cuda(), t.cuda(), m.reshape(-1).cuda(), 1, use_graph=False)
    torch.cuda.synchronize()
    assert abs(net.last_loss() - loss_r) < 1e-6 * loss_r
    assert abs(net.last_loss() - gold["loss"][0]) < 1e-6 * gold["loss"][0]
    gd = net.grads.cpu()
    offs, _ = dip_ref.param_offsets(units, 128)
    for i in range(len(units)):
        Wg, bg, gg, beg = dip_ref.views(gd, units, i, offs)
        Wr, br, gr, ber = dip_ref.views(g_r, units, i, offs)
        assert rel(Wg, Wr) < 1e-4, i
        if gg is not None:
            assert rel(gg, gr) < 1e-4 and rel(beg, ber) < 1e-4, i
        else:
            assert rel(bg, br) < 1e-4, i          # biases before a BN are rounding noise; skip those
    # first Adam move = -lr * g / (|g| + eps): identical except where a rounding-level gradient flips sign
    expect = flat.double() - 0.1 * g_r / (g_r.abs() + 1e-8)
    dp = (net.params.cpu().double() - expect).abs()
    keep = torch.ones_like(dp, dtype=torch.bool)
    for i, u in enumerate(units):                 # biases before a BN: zero gradient in exact arithmetic
        if u.bn:
            keep[offs[i][1]:offs[i][1] + u.cout] = False
    assert float((dp[keep] > 1e-4).float().mean()) < 1e-3


def test_unet_gradients_implicit_sizes_vs_fp64(L, upsample_dgrad):
    """Step-0 gradients of the U-Net at 52 x 52 (up_4 and the first convs on the implicit-GEMM
    kernels, up_4's data gradient as the effective 4 x 4 stride-2 conv + reflection border terms)
    against the fp64 restatement: 1e-4 (as at 36 x 36) or twice the fp32 torch error."""
    from gen_dip_golden import flat_params
    from lrspnp.dip import lipschitz_unet_units
    units = lipschitz_unet_units(128, 128, 128)
    H = 52
    flat = torch.from_numpy(flat_params(units, 21, 128, H, H))
    g = torch.Generator().manual_seed(5)
    x, t = torch.rand(128, H, H, generator=g), torch.rand(128, H, H, generator=g)
    m = (torch.rand(H * H, generator=g) > 0.1).float()
    net = _engine(units, flat, H, H, upsample_dgrad=upsample_dgrad)
    grads = {}
    for dt in (torch.float64, torch.float32):
        p = flat.to(dt).clone().requires_grad_(True)
        dip_ref.loss_fn(dip_ref.forward(p, units, x.to(dt)), t.to(dt), m.to(dt)).backward()
        grads[dt] = p.grad.double()
    net.train_steps(x.cuda(), t.cuda(), m.cuda(), 1, use_graph=False)
    torch.cuda.synchronize()
    gd = net.grads.cpu()
    offs, _ = dip_ref.param_offsets(units, 128, H, H)
    # 1e-4, or twice the fp32-torch error where fp32 itself is further from fp64 (the first conv's
    # weight gradient, at the end of the backward chain)
    for i in range(len(units)):
        Wg, bg, gg, beg = dip_ref.views(gd, units, i, offs, 128, H, H)
        Wr, br, gr, ber = dip_ref.views(grads[torch.float64], units, i, offs, 128, H, H)
        W32, b32, g32, be32 = dip_ref.views(grads[torch.float32], units, i, offs, 128, H, H)
        assert rel(Wg, Wr) < max(1e-4, 2 * rel(W32, Wr)), (i, rel(Wg, Wr), rel(W32, Wr))
        if gg is not None:
            assert rel(gg, gr) < max(1e-4, 2 * rel(g32, gr)) and rel(beg, ber) < max(1e-4, 2 * rel(be32, ber)), i


@pytest.mark.parametrize("H", [12, 132])
def test_workspace_alignment_offset_by_4_vs_fp64(L, H):
    """The half of a node's plan that lrs_dipnet_bind completes from the workspace's 16-byte alignment.
    A three-conv 1-Lip chain (stride-2 3 x 3, 3 x 3, 1 x 1 without BatchNorm; split-bf16) on an 8 x H x H
    input is bound twice with the same parameters, input, target and pixel mask: to an aligned workspace, and
    to a buffer of lrs_dipnet_workspace() + 16 bytes offset by 4.  Each runs 3 eager training steps; the
    third step's output and parameter gradients are compared with the fp64 restatement at the parameters
    the engine held after its second step, with the bound of test_unet_gradients_implicit_sizes_vs_fp64:
    1e-4, or twice the fp32-torch error.  (Each against the oracle, not against each other bitwise: the
    float4 kernels give way to the scalar ones.)  H = 12: 6 x 6 maps, where both BatchNorms run inside the
    direct conv launch and the alignment changes only the scalar / float4 forms inside the launchers;
    H = 132: 66 x 66 maps of 4356 pixels, where the aligned binding takes the register BatchNorm k_bn_fwd_r
    and the offset one the generic kernels."""
    from gen_dip_golden import flat_params
    from lrspnp.dip import BN_NONE, DipNet, conv_node
    C = 8
    units = [conv_node(0, 0, 16, 3, 2), conv_node(1, 0, 16, 3), conv_node(2, 0, C, 1, bn=BN_NONE)]
    Ho = H // 2
    flat = torch.from_numpy(flat_params(units, 33, C, H, H))
    g = torch.Generator().manual_seed(8)
    x, t = torch.rand(C, H, H, generator=g), torch.rand(C, Ho, Ho, generator=g)
    m = (torch.rand(Ho * Ho, generator=g) > 0.1).float()
    offs, _ = dip_ref.param_offsets(units, C, H, H)
    for shift in (0, 4):
        net = DipNet(units, C, H, H)
        if shift:
            nbytes = int(L.lrs_dipnet_workspace(net.h))
            buf = torch.zeros(nbytes + 16, dtype=torch.uint8, device="cuda")
            net.ws = buf[shift:shift + nbytes]
            assert net.ws.data_ptr() % 16 == shift
            rc = L.lrs_dipnet_bind(net.h, P(net.params), P(net.grads), P(net.exp_avg), P(net.exp_avg_sq), P(net.bnstats),
                                   P(net.ws), nbytes)
            assert rc == 0
        net.params.copy_(flat.cuda())
        net.reset_optimizer()
        net.train_steps(x.cuda(), t.cuda(), m.cuda(), 2, lr=0.01, use_graph=False)   # LrsError unless LRS_OK
        torch.cuda.synchronize()
        p2 = net.params.cpu().clone()
        net.train_steps(x.cuda(), t.cuda(), m.cuda(), 1, lr=0.01, use_graph=False)
        torch.cuda.synchronize()
        out, gd = net.output().cpu(), net.grads.cpu()
        ref = {}
        for dt in (torch.float64, torch.float32):
            p = p2.to(dt).clone().requires_grad_(True)
            o = dip_ref.forward(p, units, x.to(dt))
            dip_ref.loss_fn(o, t.to(dt), m.to(dt)).backward()
            ref[dt] = (o.detach().double(), p.grad.double())
        (o64, g64), (o32, g32) = ref[torch.float64], ref[torch.float32]
        print("shift", shift, "H", H, "out", rel(out, o64), rel(o32, o64))
        assert rel(out, o64) < max(1e-4, 2 * rel(o32, o64)), shift
        for i in range(len(units)):
            Wg, bg, gg, beg = dip_ref.views(gd, units, i, offs, C, H, H)
            Wr, br, gr, ber = dip_ref.views(g64, units, i, offs, C, H, H)
            W32, b32, ga32, be32 = dip_ref.views(g32, units, i, offs, C, H, H)
            print("  node", i, rel(Wg, Wr), rel(W32, Wr))
            assert rel(Wg, Wr) < max(1e-4, 2 * rel(W32, Wr)), (shift, i, rel(Wg, Wr), rel(W32, Wr))
            if gg is not None:
                assert rel(gg, gr) < max(1e-4, 2 * rel(ga32, gr)) and rel(beg, ber) < max(1e-4, 2 * rel(be32, ber)), (shift, i)


def _grads_vs_fp64_on_gpu(nodes, flat, x, t, m, net, c0, H, W):
    """Step-0 gradient of the engine against the restatement in fp64 and fp32 torch on the GPU (TF32
    off): per parameter tensor, (engine error, fp32-torch error) relative to fp64."""
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    grads = {}
    for dt in (torch.float64, torch.float32):
        p = flat.to(dt).cuda().clone().requires_grad_(True)
        dip_ref.loss_fn(dip_ref.forward(p, nodes, x.to(dt).cuda()), t.to(dt).cuda(), m.to(dt).cuda()).backward()
        grads[dt] = p.grad.double().cpu()
        del p
    net.train_steps(x.cuda(), t.cuda(), m.cuda(), 1, use_graph=False)
    torch.cuda.synchronize()
    gd = net.grads.cpu().double()
    offs, _ = dip_ref.param_offsets(nodes, c0, H, W)
    out = []
    for i in range(len(nodes)):
        trip = zip(dip_ref.views(gd, nodes, i, offs, c0, H, W), dip_ref.views(grads[torch.float64], nodes, i, offs, c0, H, W),
                   dip_ref.views(grads[torch.float32], nodes, i, offs, c0, H, W))
        for j, (ga, g64, g32) in enumerate(trip):
            if ga is not None:
                out.append((i, j, rel(ga, g64), rel(g32, g64)))
    return out


def test_unet_gradients_bench_size_196_vs_fp64(L):
    """BASELINE configs[2]'s DIP at its benched size: the 198 -> 128 -> 198 my_Lipschitz_Unet on
    196 x 196 (models/my_Lipschitz_Unet.py:116-148; its 196^2 / 98^2 maps run the register-resident
    BatchNorm k_bn_fwd_r / k_bn_bwd_r, the parity-class upsampled convs LdUpDgradTM / LdWgradCls +
    k_upc_wgrad_combine, k_fold_pad and the weight-gradient side stream).  Step-0 gradients of every
    parameter tensor against the fp64 restatement on the GPU: 1e-4 relative, or twice the fp32-torch
    error where fp32 itself is further from fp64 (as at 36^2 and 52^2).  Biases feeding a BN are
    rounding noise in exact arithmetic (fp32 error > 100 %) and skipped."""
    from gen_dip_golden import flat_params
    from lrspnp.dip import lipschitz_unet_units
    C, H = 198, 196
    units = lipschitz_unet_units(C, C, 128)
    flat = torch.from_numpy(flat_params(units, 41, C, H, H))
    g = torch.Generator().manual_seed(12)
    x, t = torch.rand(C, H, H, generator=g), torch.rand(C, H, H, generator=g)
    m = (torch.rand(H * H, generator=g) > 0.1).float()
    net = _engine(units, flat, H, H, C)
    res = _grads_vs_fp64_on_gpu(units, flat, x, t, m, net, C, H, H)
    worst = max(res, key=lambda r: r[2] / max(1e-4, 2 * r[3]) if r[3] <= 1.0 else 0)
    print("worst (node, tensor, engine err, fp32 err):", worst)
    for i, j, e, e32 in res:
        if e32 > 1.0:
            continue
        assert e < max(1e-4, 2 * e32), (i, j, e, e32)


def test_skip_net_gradients_config3_size_vs_fp64(L):
    """BASELINE configs[3]'s DIP at full size: the skip net on 512 x 512 x 224 (models/skip.py:5-99,
    main_LRS_PnP_DIP_pro.py:215-221).  Step-0 gradients against the fp64 restatement on the GPU with
    the bound of the 36^2 skip test: at most twice the fp32-torch error, and 2e-3 elsewhere (BN over
    the deep 32^2..16^2 maps conditions these gradients; a pre-activation within rounding of 0 may
    take the other LeakyReLU branch).  Entries that are rounding noise in exact arithmetic are
    skipped."""
    from gen_dip_golden import flat_params
    from lrspnp.dip import skip_nodes
    C, H = 224, 512
    nodes = skip_nodes(C, C)
    flat = torch.from_numpy(flat_params(nodes, 13, C, H, H))
    g = torch.Generator().manual_seed(4)
    x, t = torch.rand(C, H, H, generator=g), torch.rand(C, H, H, generator=g)
    m = (torch.rand(H * H, generator=g) > 0.05).float()
    net = _engine(nodes, flat, H, H, C)
    res = _grads_vs_fp64_on_gpu(nodes, flat, x, t, m, net, C, H, H)
    worst = max(res, key=lambda r: r[2] / max(2e-3, 2 * r[3]) if r[3] <= 1.0 else 0)
    print("worst (node, tensor, engine err, fp32 err):", worst)
    for i, j, e, e32 in res:
        if e32 > 1.0:
            continue
        assert e < max(2e-3, 2 * e32), (i, j, e, e32)


def test_nets_with_different_opts_coexist(L):
    """Per-handle modes (lrs_dip_opts, fixed at creation; no process-wide state): a split-bf16 and an
    f32 net, and a zero-padded U-Net (its upsampled convs take the effective-kernel data gradient
    when upsample_dgrad = 1) created with both modes, all interleaved in one process.  Each keeps
    its own arithmetic: step-0 gradients match the fp64 restatement, and re-running a net after the
    others gives bitwise its first result."""
    from gen_dip_golden import flat_params
    from lrspnp.dip import lipschitz_unet_units
    H = 36
    cases = []
    for pad, opts in [("reflection", dict(precision=1)), ("reflection", dict(precision=0)),
                      ("zero", dict(upsample_dgrad=1)), ("zero", dict(upsample_dgrad=0))]:
        units = lipschitz_unet_units(128, 128, 128, pad=pad)
        flat = torch.from_numpy(flat_params(units, 31, 128, H, H))
        cases.append((units, flat, _engine(units, flat, H, H, **opts), opts))
    for units, flat, net, opts in cases:
        o = _lib.DipOpts()
        assert net.L.lrs_dipnet_get_opts(net.h, ctypes.byref(o)) == 0
        assert (o.precision, o.upsample_dgrad) == (opts.get("precision", 1), opts.get("upsample_dgrad", 0))
    g = torch.Generator().manual_seed(8)
    x, t = torch.rand(128, H, H, generator=g), torch.rand(128, H, H, generator=g)
    m = (torch.rand(H * H, generator=g) > 0.1).float()
    first, flips = [], []
    for units, flat, net, _ in cases:          # one backward each, interleaved
        net.params.copy_(flat.cuda())
        net.reset_optimizer()
        net.train_steps(x.cuda(), t.cuda(), m.cuda(), 1, use_graph=False)
        torch.cuda.synchronize()
        first.append(net.grads.clone())
        # LeakyReLU branches of this forward vs the fp64 restatement's (see below)
        _, acts = dip_ref.forward(flat.double(), units, x.double(), return_all=True)
        flips.append(sum(int(((net.node_buffer(i, 0).cpu() > 0) != (acts[i][0] > 0)).sum())
                         for i in range(len(units))))
    for k, (units, flat, net, _) in enumerate(cases):
        p = flat.double().clone().requires_grad_(True)
        dip_ref.loss_fn(dip_ref.forward(p, units, x.double()), t.double(), m.double()).backward()
        p32 = flat.clone().requires_grad_(True)
        dip_ref.loss_fn(dip_ref.forward(p32, units, x), t, m).backward()
        # A pre-activation within ~1e-7 of 0 can take the other LeakyReLU branch than in fp64 (the
        # forward is ~1e-6 from fp64); one flipped pixel moves every upstream gradient by ~1e-3
        # (tools/diag_scale.py: 1 flip at node 12 -> 7e-4 for this data with the reflection net).
        # Without a flip the 1e-4 bound holds; with one, the loose bound only guards the mode.
        tol = max(1e-4, 2 * rel(p32.grad, p.grad)) if flips[k] == 0 else 5e-3
        assert rel(first[k], p.grad) < tol, (k, flips[k], rel(first[k], p.grad))
    for k, (units, flat, net, _) in enumerate(cases):   # again, after all the others ran
        net.params.copy_(flat.cuda())
        net.reset_optimizer()
        net.train_steps(x.cuda(), t.cuda(), m.cuda(), 1, use_graph=False)
        torch.cuda.synchronize()
        assert torch.equal(net.grads, first[k]), k


def test_unet_graph_replay_equals_eager(L):
    units, flat, x, t, m = _problem()
    xd, td, md = x.cuda(), t.cuda(), m.reshape(-1).cuda()
    a = _engine(units, flat)
    a.train_steps(xd, td, md, 4, use_graph=False)
    b = _engine(units, flat)
    b.train_steps(xd, td, md, 1, use_graph=True)      # capture + 1 replay
    b.train_steps(xd, td, md, 3, use_graph=True)      # replays
    torch.cuda.synchronize()
    assert torch.equal(a.params, b.params)
    assert torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    assert torch.equal(a.output(), b.output())


def test_unet_generalised_bands_196(L):
    """in = out = 198 bands, hidden 128, 196 x 196 (SURVEY.md §8 a8 generalised config)."""
    from lrspnp.dip import lipschitz_unet_units
    units = lipschitz_unet_units(198, 198, 128)
    g = torch.Generator().manual_seed(9)
    from gen_dip_golden import flat_params
    flat = torch.from_numpy(flat_params(units, 77, 198, 196, 196))
    x = torch.rand(198, 196, 196, generator=g)
    net = _engine(units, flat, 196, 196, 198)
    out = net.forward(x.cuda()).cpu()
    assert out.shape == (198, 196, 196)
    assert rel(out, dip_ref.forward(flat, units, x)) < 1e-5
    # training steps at this size (the last conv has 198 > 128 channels and no BN: its bias-gradient
    # partials must fit the workspace) — loss of the first step = the restatement's
    t = torch.rand(198, 196, 196, generator=g)
    m = (torch.rand(196 * 196, generator=g) > 0.2).float()
    loss_ref = float(dip_ref.loss_fn(dip_ref.forward(flat, units, x), t, m))
    net.train_steps(x.cuda(), t.cuda(), m.cuda(), 1, use_graph=False)
    torch.cuda.synchronize()
    assert abs(net.last_loss() - loss_ref) < 1e-5 * loss_ref
    net.train_steps(x.cuda(), t.cuda(), m.cuda(), 2, use_graph=False)
    assert np.isfinite(net.last_loss()) and net.last_loss() > 0
    assert torch.isfinite(net.params).all()


def test_lipschitz_dip_run_early_stop(L):
    from lrspnp.dip import DipConfig, LipschitzDip
    units, flat, x, t, m = _problem()
    dip = LipschitzDip(128, 36, 36, DipConfig(num_iter=400, poll_every=10))
    out = dip.run(t.cuda(), x.cuda(), m.reshape(-1).cuda(), seed=3)
    assert out.shape == (128, 36, 36) and torch.isfinite(out).all()
    assert dip.last_stop_epoch is None or dip.last_stop_epoch >= 89   # >= 30 + 60 - 1 steps
    out2 = dip.run(t.cuda(), x.cuda(), m.reshape(-1).cuda(), seed=3, num_iter=5, early_stop=False)
    assert torch.isfinite(out2).all()


def test_lipschitz_dip_adaptive_polls_equal_every_step(L):
    """DipConfig.poll_every=None (polls after the steps until the earliest possible stop) against a poll
    after every step: the same stop epoch, no step past it, the same returned output bit for bit; the
    fixed 10-step cadence stops at the same epoch too (with up to 9 steps past it)."""
    from lrspnp.dip import DipConfig, LipschitzDip
    units, flat, x, t, m = _problem()
    args = (t.cuda(), x.cuda(), m.reshape(-1).cuda())
    res = {}
    for pe in (None, 1, 10):
        dip = LipschitzDip(128, 36, 36, DipConfig(num_iter=600, poll_every=pe))
        out = dip.run(*args, seed=5)
        torch.cuda.synchronize()
        res[pe] = (dip.last_stop_epoch, dip.last_steps, out.clone())
    stop, steps, out = res[None]
    assert stop is not None and stop >= 89
    assert steps == stop + 1 and res[1][1] == stop + 1
    assert res[1][0] == stop and res[10][0] == stop
    assert torch.equal(out, res[1][2]) and torch.equal(out, res[10][2])


def test_layout_transforms_match_reference_reshapes(L):
    from lrspnp import ops
    g = np.random.default_rng(0)
    H, W, B = 12, 7, 5
    X = g.standard_normal((H * W, B)).astype(np.float32)
    L2 = g.standard_normal((H * W, B)).astype(np.float32)
    c2 = np.float32(1 / 0.1)
    # …1-LiP.py:404  (X + (1/mu_2)*lambda_2).numpy().transpose(1,0).reshape((B,W,H)).transpose((0,2,1))
    ref_in = (X + c2 * L2).transpose(1, 0).reshape((B, W, H)).transpose((0, 2, 1))
    got = ops.unfolded_to_image(torch.from_numpy(X).cuda(), torch.from_numpy(L2).cuda(), float(c2), H, W)
    np.testing.assert_array_equal(got.cpu().numpy(), ref_in)
    img = g.standard_normal((B, H, W)).astype(np.float32)
    # :411  U.numpy().transpose(0,1,3,2).reshape(B,-1).transpose(1,0)
    ref_U = img[None].transpose(0, 1, 3, 2).reshape(B, -1).transpose(1, 0)
    got_U = ops.image_to_unfolded(torch.from_numpy(img).cuda(), H, W)
    np.testing.assert_array_equal(got_U.cpu().numpy(), ref_U)


def test_solver_dip_mode_runs(L, golden):
    """One LRS-PnP-DIP(1-Lip) outer iteration on the native 36x36x128 data (img5 + lrs_mask):
    fro4 ISTA (Nit 100) beside the DIP prox, then the X / dual update."""
    from lrspnp import LrsPnP, LrsPnPConfig
    from lrspnp.data import mask_matrix, synthetic_dictionary, unfold
    from lrspnp.dip import DipConfig
    from lrspnp.metrics import mpsnr
    d = golden("data_img5.npz")
    noisy, clean, mask = d["noisy_img5"][0], d["clean_img5"][0], d["lrs_mask"]
    Y, M = unfold(noisy), mask_matrix(mask, 128)
    cfg = LrsPnPConfig.dip_1lip(dip=DipConfig(num_iter=300, poll_every=10))
    s = LrsPnP(Y, M, synthetic_dictionary(1296, 256, 0), cfg, image_shape=(36, 36))
    clean_d = torch.from_numpy(np.ascontiguousarray(clean)).cuda()
    p0 = mpsnr(s.X, clean_d)
    s.step()
    torch.cuda.synchronize()
    assert torch.isfinite(s.X).all() and torch.isfinite(s.U).all()
    steps, stop = s.dip_steps[0]
    assert 90 <= steps <= 300
    p1 = mpsnr(s.X, clean_d)
    assert np.isfinite(p1) and p1 > p0 - 3.0


def test_skip_net_forward_step_vs_reference(L, golden):
    """models/skip.py net of main_LRS_PnP_DIP_pro.py (Concat with centre crop, plain BN, Sigmoid):
    forward and first-step loss vs the reference module's outputs, gradients vs fp64 torch."""
    from gen_dip_golden import flat_params, problem
    from lrspnp.dip import skip_nodes
    gold = golden("skip_golden.npz")
    nodes = skip_nodes(128, 128)
    flat = torch.from_numpy(flat_params(nodes, int(gold["seed"])))
    x, t, m = (torch.from_numpy(a) for a in problem(int(gold["seed"])))
    net = _engine(nodes, flat)
    out = net.forward(x.cuda()).cpu()
    sub = int(gold["sub"])
    assert rel(out.reshape(-1)[::sub], torch.from_numpy(gold["out_sub"][0])) < 1e-5
    grads = {}
    for dt in (torch.float64, torch.float32):
        p = flat.to(dt).clone().requires_grad_(True)
        dip_ref.loss_fn(dip_ref.forward(p, nodes, x.to(dt)), t.to(dt), m.reshape(-1).to(dt)).backward()
        grads[dt] = p.grad.double()
    net.train_steps(x.cuda(), t.cuda(), m.reshape(-1).cuda(), 1, use_graph=False)
    torch.cuda.synchronize()
    assert abs(net.last_loss() - gold["loss"][0]) < 1e-6 * gold["loss"][0]
    gd = net.grads.cpu().double()
    offs, _ = dip_ref.param_offsets(nodes, 128)
    # BatchNorm over the 2x2 / 3x3 maps of the deep scales makes these gradients ill-conditioned:
    # fp32 CPU torch itself is ~5e-3 from fp64.  The engine must be no further from fp64 than
    # twice that, and within 2e-3 elsewhere: a pre-activation within rounding of 0 can take the
    # other LeakyReLU branch in fp32 (slope 1 vs 0.2), which moves one channel's row of dW by
    # ~1e-3 of the matrix norm (seen once at node 34, channel 81, on MI355X).  Entries that are
    # rounding noise in exact arithmetic (biases / betas feeding a BN, fp32 error > 100 %) are
    # skipped.
    for i in range(len(nodes)):
        trip = zip(dip_ref.views(gd, nodes, i, offs), dip_ref.views(grads[torch.float64], nodes, i, offs),
                   dip_ref.views(grads[torch.float32], nodes, i, offs))
        for j, (ga, g64, g32) in enumerate(trip):
            if ga is None:
                continue
            e32 = rel(g32, g64)
            if e32 > 1.0:
                continue
            assert rel(ga, g64) < max(2e-3, 2.0 * e32), (i, j, rel(ga, g64), e32)


def test_skip_net_generalised_bands(L):
    """skip net with 198 bands on a ragged 50 x 44 map (any H, W: Concat crops);
    the literal 200 x 200 x 198 size is test_skip_net_literal_config2_cube."""
    from gen_dip_golden import flat_params
    from lrspnp.dip import skip_nodes
    nodes = skip_nodes(198, 198)
    flat = torch.from_numpy(flat_params(nodes, 5, 198, 50, 44))
    x = torch.rand(198, 50, 44, generator=torch.Generator().manual_seed(2))
    net = _engine(nodes, flat, 50, 44, 198)
    out = net.forward(x.cuda()).cpu()
    assert out.shape == (198, 50, 44)
    assert rel(out, dip_ref.forward(flat, nodes, x)) < 1e-5


def test_skip_net_literal_config2_cube(L):
    """The skip net on BASELINE configs[2]'s literal 200 x 200 x 198 cube (bench.py --workload dip-pro
    --cube 200x200x198): forward vs the fp32 restatement on the GPU at 1e-5, step-0 loss at 1e-5."""
    from gen_dip_golden import flat_params
    from lrspnp.dip import skip_nodes
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    C, H = 198, 200
    nodes = skip_nodes(C, C)
    flat = torch.from_numpy(flat_params(nodes, 17, C, H, H))
    g = torch.Generator().manual_seed(6)
    x, t = torch.rand(C, H, H, generator=g), torch.rand(C, H, H, generator=g)
    m = (torch.rand(H * H, generator=g) > 0.05).float()
    net = _engine(nodes, flat, H, H, C)
    out = net.forward(x.cuda())
    with torch.no_grad():
        ref = dip_ref.forward(flat.cuda(), nodes, x.cuda())
        loss_r = float(dip_ref.loss_fn(ref, t.cuda(), m.cuda()))
    assert out.shape == ref.shape == (C, H, H)
    assert rel(out, ref) < 1e-5
    net.train_steps(x.cuda(), t.cuda(), m.cuda(), 1, use_graph=False)
    torch.cuda.synchronize()
    assert abs(net.last_loss() - loss_r) < 1e-5 * loss_r


def test_skip_net_config3_full_size(L):
    """BASELINE configs[3]'s DIP at full size: the skip net (5 x 128 channels, 128-ch skips, Sigmoid)
    on a 512 x 512 x 224 cube (main_LRS_PnP_DIP_pro.py:215-221 with 224 bands): the engine's forward
    against the plain-torch fp32 restatement run on the GPU (TF32 off) at 1e-5 relative L2, and the
    step-0 masked-MSE loss at 1e-5."""
    from gen_dip_golden import flat_params
    from lrspnp.dip import skip_nodes
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    C, H = 224, 512
    nodes = skip_nodes(C, C)
    flat = torch.from_numpy(flat_params(nodes, 11, C, H, H))
    g = torch.Generator().manual_seed(3)
    x = torch.rand(C, H, H, generator=g)
    t = torch.rand(C, H, H, generator=g)
    m = (torch.rand(H * H, generator=g) > 0.05).float()
    net = _engine(nodes, flat, H, H, C)
    out = net.forward(x.cuda())
    with torch.no_grad():
        ref = dip_ref.forward(flat.cuda(), nodes, x.cuda())
        loss_r = float(dip_ref.loss_fn(ref, t.cuda(), m.cuda()))
    assert out.shape == ref.shape == (C, H, H)
    assert rel(out, ref) < 1e-5
    net.train_steps(x.cuda(), t.cuda(), m.cuda(), 1, use_graph=False)
    torch.cuda.synchronize()
    assert abs(net.last_loss() - loss_r) < 1e-5 * loss_r


def test_solver_dip_pro_skip_runs(L, golden):
    """One LRS-PnP-DIP(pro) outer iteration: the skip net as the low-rank prox (…pro.py:399-420)."""
    from lrspnp import LrsPnP, LrsPnPConfig
    from lrspnp.data import mask_matrix, synthetic_dictionary, unfold
    from lrspnp.dip import DipConfig
    d = golden("data_img5.npz")
    noisy, mask = d["noisy_img5"][0], d["lrs_mask"]
    cfg = LrsPnPConfig.dip_pro(dip=DipConfig(net="skip", num_iter=40, early_stop=False))
    s = LrsPnP(unfold(noisy), mask_matrix(mask, 128), synthetic_dictionary(1296, 256, 0), cfg, image_shape=(36, 36))
    s.step()
    torch.cuda.synchronize()
    assert torch.isfinite(s.X).all() and torch.isfinite(s.U).all()
    assert float(s.U.min()) >= 0.0 and float(s.U.max()) <= 1.0      # Sigmoid output
    assert s.dip_steps[0] == (40, None)


def test_mssim_matches_torch_restatement(L):
    """lrs_ssim_f32 vs the pytorch_ssim formula (pytorch_ssim/__init__.py:7-37) in torch fp64."""
    import math
    from lrspnp.metrics import mssim
    g = torch.Generator().manual_seed(8)
    a = torch.rand(7, 36, 29, generator=g)
    b = (a + 0.1 * torch.randn(7, 36, 29, generator=g)).clamp(0, 1)
    gauss = torch.tensor([math.exp(-(x - 5) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)])
    gauss = gauss / gauss.sum()
    win = (gauss[:, None] @ gauss[None, :]).double().expand(7, 1, 11, 11)
    A, Bt = a.double()[None], b.double()[None]
    conv = lambda t: F.conv2d(t, win, padding=5, groups=7)
    mu1, mu2 = conv(A), conv(Bt)
    s1, s2, s12 = conv(A * A) - mu1 ** 2, conv(Bt * Bt) - mu2 ** 2, conv(A * Bt) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    ref = (((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 ** 2 + mu2 ** 2 + C1) * (s1 + s2 + C2))).mean()
    got = mssim(a.cuda(), b.cuda())
    assert abs(got - float(ref)) < 1e-5
    assert abs(mssim(a.cuda(), a.cuda()) - 1.0) < 1e-6


@pytest.mark.parametrize("C,H,W", [(3, 4, 13), (40, 232, 232)])
def test_mssim_small_and_large_images(L, C, H, W):
    """lrs_ssim_f32 on images smaller than the 11 x 11 window (every window hangs over the zero border)
    and on C H W = 2152960 > 8192 * 256 elements, against the fp64 restatement and at the 1e-5 of
    test_mssim_matches_torch_restatement."""
    import math
    from lrspnp.metrics import mssim
    g = torch.Generator().manual_seed(C)
    a = torch.rand(C, H, W, generator=g)
    b = (a + 0.1 * torch.randn(C, H, W, generator=g)).clamp(0, 1)
    gauss = torch.tensor([math.exp(-(x - 5) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)])
    gauss = gauss / gauss.sum()
    win = (gauss[:, None] @ gauss[None, :]).double().expand(C, 1, 11, 11)
    A, Bt = a.double()[None], b.double()[None]
    conv = lambda t: F.conv2d(t, win, padding=5, groups=C)
    mu1, mu2 = conv(A), conv(Bt)
    s1, s2, s12 = conv(A * A) - mu1 ** 2, conv(Bt * Bt) - mu2 ** 2, conv(A * Bt) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    ref = (((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 ** 2 + mu2 ** 2 + C1) * (s1 + s2 + C2))).mean()
    got = mssim(a.cuda(), b.cuda())
    assert abs(got - float(ref)) < 1e-5, (got, float(ref))
    assert abs(mssim(a.cuda(), a.cuda()) - 1.0) < 1e-6

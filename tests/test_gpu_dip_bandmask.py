"""GPU: band-varying observation masks in the DIP low-rank prox: a per-element mask [C][P] in the
three loss heads (k_masked_mse, k_mse_head, k_pw's fused head), lrs_masked_mse_cmask_f32,
lrs_dipnet_train_steps_cmask, DipNet / DipProx and the solver's plumbing.

References are formed here in fp64 torch: loss = F.mse_loss(target*m, out*m) on dip_ref.forward's
output (dip_ref.loss_fn views its mask as (1, H, W) and cannot take a per-element one).
Tolerances: stand-alone masked MSE 1e-6 (loss relative, gout of max|gout|); whole-net
step-0 loss 1e-6, gradients 1e-4 relative L2 or twice the fp32-torch error where that is larger.
Conv biases that feed a BatchNorm have zero gradient in exact arithmetic (rounding noise in every
precision) and are not compared, as in tests/test_gpu_dip.py.

The three nets reach the three heads: (a) the 1-Lip U-Net at 36x36x8 (k_pw's fused head, P <= 4096),
(b) the same at 68x68 (k_mse_head; 68 is the smallest size above 64 = sqrt(4096) the U-Net maps to
itself: 36, 52, 68, ...), (c) a 3-conv chain whose last conv carries a BatchNorm at 20x20 (the
generic k_masked_mse + BN backward).  Net (c) has 2 output bands: k_masked_mse adds one fp64 loss
partial per workgroup (here one per band) with atomics, and only a sum of two addends is the same in
either arrival order, so the loss can be compared bit for bit.
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
    return _lib.device_lib()


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- the three nets -----------------------------------------------------------------------------
# name -> (C, H, stripe_mask seed, missing band): the masks tests/test_bandmask_host.py checks
NETS = {"pw_head_36": (8, 36, 3, 5), "mse_head_68": (8, 68, 4, 2), "generic_bn_20": (2, 20, 5, 1)}


def _nodes(name):
    from lrspnp.dip import BN_LIP, conv_node, lipschitz_unet_nodes, unet_size_ok
    C, H, _, _ = NETS[name]
    if name == "generic_bn_20":
        return [conv_node(0, 0, 16, 3), conv_node(1, 0, 16, 3), conv_node(2, 0, C, 1, bn=BN_LIP)]
    assert unet_size_ok(H, H)
    if name == "mse_head_68":   # the smallest self-reproducing size above the fused head's 4096 pixels
        assert H * H > 4096 and not any(unet_size_ok(h, h) for h in range(65, H))
    return lipschitz_unet_nodes(C, C, 128)


_PROBLEMS = {}


def _problem(name):
    """Nodes, seeded parameters, input, target and the band-varying mask (with a missing band) of a net;
    built once and shared (never modified)."""
    if name not in _PROBLEMS:
        from gen_dip_golden import flat_params
        from lrspnp.data import stripe_mask
        C, H, seed, mb = NETS[name]
        nodes = _nodes(name)
        flat = torch.from_numpy(flat_params(nodes, 50 + seed, C, H, H))
        g = torch.Generator().manual_seed(seed)
        x, t = torch.rand(C, H, H, generator=g), torch.rand(C, H, H, generator=g)
        m = torch.from_numpy(stripe_mask(H, H, C, seed, missing_band=mb))
        _PROBLEMS[name] = (nodes, flat, x.cuda(), t.cuda(), m.cuda())
    return _PROBLEMS[name]


def _engine(name):
    from lrspnp.dip import DipNet
    C, H, _, _ = NETS[name]
    nodes, flat = _problem(name)[:2]
    net = DipNet(nodes, C, H, H)
    net.params.copy_(flat.cuda())
    net.reset_optimizer()
    return net


def _state(net):
    """Everything one training step leaves: loss, dL/dz and dL/dout of the last node, every parameter
    gradient, the parameters after Adam and its moments."""
    torch.cuda.synchronize()
    n = len(net.nodes) - 1
    bufs = [net.node_buffer(n, w) for w in (2, 3)]
    return dict(loss=net.last_loss(), gz=bufs[0], gout=bufs[1], grads=net.grads.clone(), params=net.params.clone(),
                m=net.exp_avg.clone(), v=net.exp_avg_sq.clone(), out=net.output().clone())


def _same(a, b):
    assert a["loss"] == b["loss"], (a["loss"], b["loss"])
    for k in ("gz", "gout", "grads", "params", "m", "v", "out"):
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert torch.equal(a[k], b[k]), k


# ---- 1. stand-alone masked MSE, per-element mask ---------------------------------------------------
@pytest.mark.parametrize("C,Px", [(3, 37), (5, 64), (2, 4100), (1, 16)])
def test_masked_mse_per_element_mask(L, C, Px):
    """lrs_masked_mse_cmask_f32 with a [C][P] mask against torch fp64: the scalar path (P % 4 != 0), the
    float4 path, more than one chunk per channel, and C = 1 where the two modes coincide.  A different
    random binary pattern per channel; the last channel's mask is all zero and its gout exactly 0."""
    from lrspnp import ops
    g = torch.Generator().manual_seed(100 + C)
    out, tgt = torch.randn(C, Px, generator=g), torch.randn(C, Px, generator=g)
    mask = (torch.rand(C, Px, generator=g) > 0.3).float()
    if C > 1:
        mask[C - 1] = 0.0
        assert not torch.equal(mask[0], mask[1]) or C == 2
    o = out.double().requires_grad_(True)
    loss = F.mse_loss(tgt.double() * mask.double(), o * mask.double())
    loss.backward()
    acc = torch.zeros(1, dtype=torch.float64, device="cuda")
    gout = torch.full((C, Px), float("nan"), device="cuda")
    od, td, md = out.cuda(), tgt.cuda(), mask.cuda()
    assert L.lrs_masked_mse_cmask_f32(P(od), P(td), P(md), C, C, Px, P(gout), P(acc), S()) == 0
    torch.cuda.synchronize()
    got, want = float(acc) / (C * Px), float(loss.detach())
    gmax = float(o.grad.abs().max())
    err = float((gout.cpu().double() - o.grad).abs().max())
    print(f"C={C} P={Px}: loss rel {abs(got - want) / want:.2e}, gout max err / max|gout| {err / gmax:.2e}")
    assert abs(got - want) <= 1e-6 * want
    assert err <= 1e-6 * gmax
    if C > 1:
        assert float(gout[C - 1].abs().max()) == 0.0
    # the Python wrapper picks the mode from the element count (and the loss without a gradient buffer)
    l2, g2 = ops.masked_mse(od, td, md)
    l3, g3 = ops.masked_mse(od, td, md.reshape(-1), want_grad=False)
    torch.cuda.synchronize()
    assert torch.equal(g2, gout) and g3 is None
    assert abs(float(l2) - want) <= 1e-6 * want and abs(float(l3) - want) <= 1e-6 * want
    if C == 1:   # [1][P] is [P]: the existing entry point gives the same bits
        acc1 = torch.zeros(1, dtype=torch.float64, device="cuda")
        gout1 = torch.empty(C, Px, device="cuda")
        assert L.lrs_masked_mse_f32(P(od), P(td), P(md), C, Px, P(gout1), P(acc1), S()) == 0
        torch.cuda.synchronize()
        assert torch.equal(gout1, gout) and float(acc1) == float(acc)


# ---- 2. bit identity of the two modes --------------------------------------------------------------
@pytest.mark.parametrize("name", list(NETS))
def test_uniform_per_element_mask_is_bit_identical_to_pixel_mask(L, name):
    """A [C][P] mask whose C rows are one pixel mask against the [P] call on the same data, through one
    training step on each head: loss, dL/dz / dL/dout of the last node, every parameter gradient and the
    parameters and moments after Adam are the same bits; two more steps stay identical."""
    nodes, flat, x, t, m = _problem(name)
    C, H, _, _ = NETS[name]
    pix = m[0].contiguous()                       # (H, W)
    full = pix.expand(C, H, H).contiguous()       # the same mask in every band
    a, b = _engine(name), _engine(name)
    assert a.mask_channels(pix) == 1 and a.mask_channels(pix.reshape(-1)) == 1 and b.mask_channels(full) == C
    a.train_steps(x, t, pix.reshape(-1), 1)
    b.train_steps(x, t, full, 1)
    sa, sb = _state(a), _state(b)
    assert sa["gz"] is not None or sa["gout"] is not None
    _same(sa, sb)
    a.train_steps(x, t, pix, 2)
    b.train_steps(x, t, full, 2)
    _same(_state(a), _state(b))
    # the stand-alone kernel too (dL/dout; its loss is an atomic sum over workgroups, not compared here)
    from lrspnp import ops
    _, g1 = ops.masked_mse(sa["out"], t, pix)
    _, g2 = ops.masked_mse(sa["out"], t, full)
    torch.cuda.synchronize()
    assert torch.equal(g1, g2)


def test_graph_replay_recaptures_on_mask_mode(L):
    """Net (a) under hipGraph replay: [P] steps, then the [C][P] mask on the same handle (other bits in
    the result, so a stale graph would show), each equal to eager; and a [C][P] view of one buffer
    passed first as [P] (its band 0) then as [C][P] at the same pointer re-captures."""
    name = "pw_head_36"
    nodes, flat, x, t, m = _problem(name)
    C, H, _, _ = NETS[name]
    pix = m[0].reshape(-1)          # band 0's mask: same pointer as m, P elements
    assert pix.data_ptr() == m.data_ptr()
    e, g = _engine(name), _engine(name)
    e.train_steps(x, t, pix, 2, use_graph=False)
    g.train_steps(x, t, pix, 1, use_graph=True)     # capture + replay
    g.train_steps(x, t, pix, 1, use_graph=True)     # replay
    _same(_state(e), _state(g))
    e.train_steps(x, t, m, 2, use_graph=False)
    g.train_steps(x, t, m, 1, use_graph=True)       # same pointers, other mask mode: re-captured
    g.train_steps(x, t, m, 1, use_graph=True)
    sg = _state(g)
    _same(_state(e), sg)
    # and the steps with the full mask did something else than two more band-0 steps would have
    e2 = _engine(name)
    e2.train_steps(x, t, pix, 4, use_graph=False)
    torch.cuda.synchronize()
    assert not torch.equal(e2.params, sg["params"])
    # uniform rows under replay: bit-identical to the [P] replay
    full = m[0].expand(C, H, H).contiguous()
    g1, g2 = _engine(name), _engine(name)
    g1.train_steps(x, t, m[0].contiguous(), 3, use_graph=True)
    g2.train_steps(x, t, full, 3, use_graph=True)
    _same(_state(g1), _state(g2))


# ---- 3. step-0 gradients with a genuinely band-varying mask ----------------------------------------
def _ref_grads(nodes, flat, x, t, m, dt):
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    p = flat.to(dt).cuda().clone().requires_grad_(True)
    out = dip_ref.forward(p, nodes, x.to(dt))
    mm = m.to(dt).view(-1, *out.shape[1:])       # (C, H, W), or (1, H, W) for a pixel mask
    loss = F.mse_loss(t.to(dt) * mm, out * mm)
    loss.backward()
    return float(loss.detach()), p.grad.double().cpu()


@pytest.mark.parametrize("name", list(NETS))
def test_step0_gradients_band_varying_mask_vs_fp64(L, name):
    """stripe_mask with a missing band through each head: loss and every parameter tensor's gradient
    against the fp64 restatement, and far from what band 0's mask broadcast over the bands gives (the
    behaviour before per-element masks), so the test cannot pass on the broadcast."""
    nodes, flat, x, t, m = _problem(name)
    C, H, _, mb = NETS[name]
    assert float(m[mb].sum()) == 0.0 and not torch.equal(m[0], m[1])
    loss64, g64 = _ref_grads(nodes, flat, x, t, m, torch.float64)
    _, g32 = _ref_grads(nodes, flat, x, t, m, torch.float32)
    _, gb0 = _ref_grads(nodes, flat, x, t, m[0], torch.float64)     # band 0's mask for every band
    net = _engine(name)
    net.train_steps(x, t, m, 1)
    torch.cuda.synchronize()
    loss = net.last_loss()
    print(f"{name}: loss rel err {abs(loss - loss64) / loss64:.2e}")
    assert abs(loss - loss64) <= 1e-6 * loss64
    gd = net.grads.cpu().double()
    offs, _ = dip_ref.param_offsets(nodes, C, H, H)
    names = ("W", "bias", "gamma", "beta")
    far = 0.0
    for i, nd in enumerate(nodes):
        trip = zip(dip_ref.views(gd, nodes, i, offs, C, H, H), dip_ref.views(g64, nodes, i, offs, C, H, H),
                   dip_ref.views(g32, nodes, i, offs, C, H, H), dip_ref.views(gb0, nodes, i, offs, C, H, H))
        for j, (ga, gr, gf, gb) in enumerate(trip):
            if ga is None or (j == 1 and nd.bn):   # a bias feeding a BatchNorm: zero in exact arithmetic
                continue
            e, e32, eb = rel(ga, gr), rel(gf, gr), rel(gb, gr)
            print(f"  node {i} {names[j]}: engine {e:.2e} fp32 torch {e32:.2e} band-0 broadcast {eb:.2e}")
            assert e < max(1e-4, 2 * e32), (i, j, e, e32)
            far = max(far, eb)
            # the broadcast is off by at least an order of magnitude more than the tolerance, in every tensor
            assert eb > 10 * max(1e-4, 2 * e32), (i, j, eb, e32)
            assert rel(ga, gb) > 10 * max(1e-4, 2 * e32), (i, j)
    # ... and by a share of the gradient itself where the loss enters (a whole band differs)
    assert far > 0.05


# ---- 4. solver plumbing ----------------------------------------------------------------------------
def _solver(M, Y=None):
    from lrspnp import LrsPnP, LrsPnPConfig
    from lrspnp.data import synthetic_cube, synthetic_dictionary, unfold
    from lrspnp.dip import DipConfig
    obs, _, _ = synthetic_cube(36, 36, 8, seed=2)
    cfg = LrsPnPConfig.dip_1lip(bb=8, sliding=8, Nit=10, dip_seed=9, dip=DipConfig(num_iter=4, early_stop=False))
    Yf = unfold(obs) if Y is None else Y
    return LrsPnP(Yf * M, M, synthetic_dictionary(64, 256, 0), cfg, image_shape=(36, 36))


def test_solver_passes_band_varying_mask_to_the_dip(L):
    from lrspnp import ops
    from lrspnp.data import mask_matrix, stripe_mask, unfold
    mask = stripe_mask(36, 36, 8, 7, missing_band=6)
    M = unfold(mask)
    s = _solver(M)
    assert tuple(s.dip_mask.shape) == (8, 36, 36)
    assert s.dip_mask.cpu().numpy().tobytes() == mask.tobytes()
    s.step()
    torch.cuda.synchronize()
    U = s.U.clone()
    assert torch.isfinite(U).all()
    dip_in, target = s.dip_in.clone(), s.dip_target.clone()
    full = torch.from_numpy(mask).cuda()
    direct = ops.image_to_unfolded(s.dip.run(target, dip_in, full, seed=9, early_stop=False), 36, 36)
    torch.cuda.synchronize()
    assert torch.equal(U, direct)
    # band 0's mask for every band (M[:, :1] broadcast) trains another net
    b0 = ops.image_to_unfolded(s.dip.run(target, dip_in, full[0].contiguous(), seed=9, early_stop=False), 36, 36)
    torch.cuda.synchronize()
    assert not torch.equal(U, b0)
    assert float((U - b0).norm() / b0.norm()) > 1e-3
    # a band-uniform M keeps the (P,) mask and the [P] path
    pix = mask[0]
    su = _solver(mask_matrix(pix, 8))
    assert tuple(su.dip_mask.shape) == (36 * 36,)
    assert torch.equal(su.dip_mask.view(36, 36).cpu(), torch.from_numpy(pix))
    su.step()
    torch.cuda.synchronize()
    d2 = ops.image_to_unfolded(su.dip.run(su.dip_target.clone(), su.dip_in.clone(), su.dip_mask, seed=9,
                                          early_stop=False), 36, 36)
    torch.cuda.synchronize()
    assert torch.equal(su.U, d2)


# ---- 5. refusals -------------------------------------------------------------------------------------
def test_bad_mask_channel_counts_are_refused_before_any_launch(L):
    from lrspnp.dip import DipProx, DipConfig
    name = "pw_head_36"
    nodes, flat, x, t, m = _problem(name)
    net = _engine(name)
    torch.cuda.synchronize()
    before = (net.params.clone(), net.grads.clone(), net.ws.clone())
    f = ctypes.c_float
    st = ctypes.c_void_p(net.stream.cuda_stream)
    for mc in (2, 0, 9):
        rc = net.L.lrs_dipnet_train_steps_cmask(net.h, P(x), P(t), P(m), mc, f(0.1), f(0.9), f(0.999), f(1e-8), None,
                                                None, 1, 0, st)
        assert rc == -1, mc
    torch.cuda.synchronize()
    # nothing was enqueued: parameters, gradients and the whole workspace (loss, step counter, ...) untouched
    assert torch.equal(net.params, before[0]) and torch.equal(net.grads, before[1]) and torch.equal(net.ws, before[2])
    acc = torch.zeros(1, dtype=torch.float64, device="cuda")
    gout = torch.zeros_like(t)
    assert L.lrs_masked_mse_cmask_f32(P(x), P(t), P(m), 2, 8, 36 * 36, P(gout), P(acc), S()) == -1
    torch.cuda.synchronize()
    assert float(acc) == 0.0 and float(gout.abs().max()) == 0.0
    prox = DipProx(8, 36, 36, DipConfig(num_iter=1, early_stop=False))
    bad = torch.ones(8 * 36 * 36 + 1, device="cuda")
    with pytest.raises(_lib.LrsError, match=r"\(1296,\).*\(8, 36, 36\)"):
        prox.run(t, x, bad, seed=0, early_stop=False)
    assert prox.calls == 0
    with pytest.raises(_lib.LrsError):
        net.train_steps(x, t, torch.ones(2, 36, 36, device="cuda"), 1)

"""GPU: the Deep Decoder low-rank prox (LRS_NODE_DECODE, csrc/dip_up.h, DipConfig.net = 'decoder').

1. the two upsampling kernels alone against F.interpolate(bilinear, align_corners=False) + activation and
   its autograd in fp64; 2. the net at step 0 against the reference module's golden and the fp64 restatement
   (tests/decoder_ref.py), under a [P] mask, a per-band [C][P] mask and none; 3. determinism and graph replay;
   4. one Adam step; 5. DipProx (plain, framed, early stopping), the solver, training sanity; 6. the
   lrspnp.nn.decodernw drop-in.

Tolerances: kernels 1e-6 of max|y| forward (<= 4 terms, exact weights), 1e-5 of max|gy| backward (<= 16
terms, the project's conv tolerance); nets: output 1e-5, loss 1e-6, gradients 1e-4 or twice the fp32-torch
error (the project's rule for whole nets).
"""
import ctypes
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
F = torch.nn.functional

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decoder_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

ACT_NONE, ACT_LRELU, ACT_SIGMOID, ACT_RELU = 0, 1, 2, 3


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


def rel(a, b):
    a = torch.as_tensor(a).double().cpu(); b = torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-300))


# ---- 1. the upsampling kernels alone ------------------------------------------------------------------
UP_SHAPES = [(1, 1, 1), (3, 1, 5), (5, 2, 3), (16, 9, 9), (7, 17, 33)]


def _up_input(shape, seed=0):
    """Normal values, negatives included, with exact zeros: scattered ones and, where the map is large
    enough, a block whose upsampled interior is exactly zero (the activation's a = 0 case)."""
    g = torch.Generator().manual_seed(seed + shape[0] * 10007 + shape[1] * 101 + shape[2])
    x = torch.randn(shape, generator=g)
    if x.numel() > 1:
        x[torch.rand(shape, generator=g) < 0.15] = 0.0
    if shape[1] >= 9 and shape[2] >= 9:
        x[:, 2:7, 3:8] = 0.0
    return x


def _ref_act(z, act):
    return torch.relu(z) if act == ACT_RELU else F.leaky_relu(z, 0.2) if act == ACT_LRELU else z


def _up_fwd(L, x, act):
    C, H, W = x.shape
    y = torch.full((C, 2 * H, 2 * W), float("nan"), device="cuda")
    assert L.lrs_up2_bilinear_act_fwd_f32(P(x), C, H, W, act, P(y), S()) == 0
    return y


def _up_bwd(L, gy, y, act):
    C, H, W = y.shape[0], y.shape[1] // 2, y.shape[2] // 2
    gx = torch.full((C, H, W), float("nan"), device="cuda")
    assert L.lrs_up2_bilinear_act_bwd_f32(P(gy), P(y), C, H, W, act, P(gx), S()) == 0
    return gx


@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU, ACT_LRELU])
@pytest.mark.parametrize("shape", UP_SHAPES)
def test_up2_kernels_vs_interpolate_fp64(L, shape, act):
    x = _up_input(shape)
    x64 = x.double().requires_grad_(True)
    ref = _ref_act(F.interpolate(x64[None], scale_factor=2, mode="bilinear", align_corners=False)[0], act)
    y = _up_fwd(L, x.cuda().contiguous(), act)
    torch.cuda.synchronize()
    ymax = float(ref.detach().abs().max())
    ef = float((y.cpu().double() - ref.detach()).abs().max())
    print("fwd", shape, act, ef, ymax)
    assert ef <= 1e-6 * ymax
    if shape == (1, 1, 1):   # every tap clamped: the input itself, bit for bit
        assert torch.equal(y.cpu(), _ref_act(x, act).expand(1, 2, 2))
    if act != ACT_NONE and shape[1] >= 9:
        assert int((y == 0).sum()) > 0   # a = 0 occurs: the derivative there is taken below
    g = torch.Generator().manual_seed(7)
    gy = torch.randn(ref.shape, generator=g)
    ref.backward(gy.double())
    gx = _up_bwd(L, gy.cuda().contiguous(), y, act)
    torch.cuda.synchronize()
    eb = float((gx.cpu().double() - x64.grad).abs().max())
    print("bwd", shape, act, eb, float(gy.abs().max()))
    assert eb <= 1e-5 * float(gy.abs().max())


@pytest.mark.parametrize("shape", UP_SHAPES)
def test_up2_adjoint_identity(L, shape):
    """<up2(x), g> = <x, up2^T(g)> (act NONE), both sides summed in fp64."""
    x = _up_input(shape, 1).cuda().contiguous()
    y = _up_fwd(L, x, ACT_NONE)
    g = torch.randn(y.shape, generator=torch.Generator().manual_seed(11)).cuda()
    gx = _up_bwd(L, g, y, ACT_NONE)
    torch.cuda.synchronize()
    lhs, rhs = float((y.double() * g.double()).sum()), float((x.double() * gx.double()).sum())
    scale = float(y.double().norm() * g.double().norm())
    assert abs(lhs - rhs) <= 1e-5 * scale, (lhs, rhs)


def test_up2_abi_refuses(L):
    x = torch.zeros(2, 3, 3, device="cuda")
    y = torch.zeros(2, 6, 6, device="cuda")
    assert L.lrs_up2_bilinear_act_fwd_f32(P(x), 2, 3, 3, ACT_SIGMOID, P(y), S()) == -1
    assert L.lrs_up2_bilinear_act_bwd_f32(P(y), P(y), 2, 3, 3, 7, P(x), S()) == -1
    assert L.lrs_up2_bilinear_act_fwd_f32(None, 2, 3, 3, ACT_RELU, P(y), S()) == -1
    assert L.lrs_up2_bilinear_act_fwd_f32(P(x), 2, 0, 3, ACT_RELU, P(y), S()) == -1


# ---- 2. the net at step 0 -----------------------------------------------------------------------------
def _golden():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decoder_golden.npz")
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _seeded_flat(nodes, c0, seed):
    """Conv weights U(+-1/sqrt(cin)) (nn.Conv2d's default scale), gamma = 1 + 0.25 u, beta = 0.1 u."""
    offs, total = R.param_offsets(nodes, c0)
    ch = R.channels(nodes, c0)
    rng = np.random.default_rng(seed)
    flat = np.zeros(total, np.float32)
    for i, (d, (w, _, g, be)) in enumerate(zip(R.node_dicts(nodes), offs)):
        co, ci = ch[i + 1], ch[d["in0"]]
        flat[w:w + co * ci] = rng.uniform(-1, 1, co * ci) / np.sqrt(ci)
        if g >= 0:
            flat[g:g + co] = 1.0 + 0.25 * rng.uniform(-1, 1, co)
            flat[be:be + co] = 0.1 * rng.uniform(-1, 1, co)
    return torch.from_numpy(flat)


_CASES = {}


def _case(name):
    """(nodes, c0, h, w, flat, x, target) of a step-0 case, built once (CPU tensors)."""
    if name in _CASES:
        return _CASES[name]
    from lrspnp.dip import deep_decoder_nodes
    if name == "golden":
        g = _golden()
        nodes = deep_decoder_nodes(16, 8, (16, 16))
        c = (nodes, 16, 9, 9, R.flat_from_golden(g), torch.from_numpy(g["x"]), torch.from_numpy(g["target"]))
    else:
        c0, bands, ch, h, w, act, seed = {"ragged": (12, 7, (12, 20), 5, 7, "relu", 21),
                                          "lrelu": (10, 5, (10, 6), 6, 5, "lrelu", 22)}[name]
        nodes = deep_decoder_nodes(c0, bands, ch, act=act)
        rng = np.random.default_rng(seed)
        x = torch.from_numpy((rng.uniform(0, 1, (c0, h, w)) * 0.1).astype(np.float32))
        t = torch.from_numpy(rng.uniform(0, 1, (bands, 4 * h, 4 * w)).astype(np.float32))
        c = (nodes, c0, h, w, _seeded_flat(nodes, c0, seed), x, t)
    _CASES[name] = c
    return c


def _mask(name, kind):
    nodes, c0, h, w, flat, x, t = _case(name)
    C, H, W = t.shape
    if kind == "none":
        return None
    if kind == "pixel":
        if name == "golden":
            return torch.from_numpy(_golden()["mask"])
        return torch.from_numpy((np.random.default_rng(5).random((H, W)) > 0.3).astype(np.float32))
    from lrspnp.data import stripe_mask
    return torch.from_numpy(stripe_mask(H, W, C, seed=4, missing_band=True))


_REFS = {}


def _reference(name, kind):
    """{dtype: (out, loss, grad)} of the restatement on the CPU, computed once per case and mask."""
    if (name, kind) not in _REFS:
        nodes, c0, h, w, flat, x, t = _case(name)
        m = _mask(name, kind)
        _REFS[name, kind] = {dt: R.step0(flat.to(dt), nodes, x.to(dt), t.to(dt), None if m is None else m.to(dt))
                             for dt in (torch.float32, torch.float64)}
    return _REFS[name, kind]


def _engine_step0(name, kind):
    from lrspnp.dip import DipNet
    nodes, c0, h, w, flat, x, t = _case(name)
    m = _mask(name, kind)
    net = DipNet(nodes, c0, h, w)
    net.params.copy_(flat.cuda())
    net.reset_optimizer()
    xd, td = x.cuda().contiguous(), t.cuda().contiguous()
    md = None if m is None else m.cuda().contiguous()
    out = net.forward(xd).clone()
    net.train_steps(xd, td, md, 1, lr=0.0)   # lr 0: the parameters stay, the step's loss and gradients remain
    torch.cuda.synchronize()
    assert torch.equal(net.params.cpu(), flat)
    assert torch.equal(net.output(), out)
    return net, out.cpu(), net.last_loss(), net.grads.cpu().clone()


def _check_grads(nodes, c0, got, ref):
    (o32, l32, g32), (o64, l64, g64) = ref[torch.float32], ref[torch.float64]
    offs, _ = R.param_offsets(nodes, c0)
    for i in range(len(nodes)):
        for j, nm in ((0, "W"), (2, "gamma"), (3, "beta")):
            a = R.views(got, nodes, i, offs, c0)[j]
            if a is None:
                continue
            r, f = R.views(g64, nodes, i, offs, c0)[j], R.views(g32, nodes, i, offs, c0)[j]
            e, e32 = rel(a, r), rel(f, r)
            print("  node", i, nm, e, e32)
            assert e < max(1e-4, 2 * e32), (i, nm, e, e32)


@pytest.mark.parametrize("kind", ["pixel", "band", "none"])
@pytest.mark.parametrize("name", ["golden", "ragged", "lrelu"])
def test_net_step0(L, name, kind):
    nodes, c0, h, w, flat, x, t = _case(name)
    ref = _reference(name, kind)
    net, out, loss, grads = _engine_step0(name, kind)
    assert net.out_shape == tuple(t.shape)
    o64, l64, _ = ref[torch.float64]
    print(name, kind, "out", rel(out, o64), "loss", abs(loss - float(l64)) / float(l64))
    assert rel(out, o64) < 1e-5
    assert abs(loss - float(l64)) < 1e-6 * float(l64)
    _check_grads(nodes, c0, grads, ref)
    if name == "golden" and kind == "pixel":   # the reference module's own numbers
        g = _golden()
        assert rel(out, g["out64"]) < 1e-5
        assert abs(loss - float(g["loss64"])) < 1e-6 * float(g["loss64"])
        off = 0
        for n in g["param_names"]:
            r = torch.from_numpy(g["g64/" + str(n)]).reshape(-1)
            f = torch.from_numpy(g["g32/" + str(n)]).reshape(-1)
            assert rel(grads[off:off + r.numel()], r) < max(1e-4, 2 * rel(f, r)), n
            off += r.numel()


# ---- 3. determinism -----------------------------------------------------------------------------------
def _train5(name, use_graph):
    from lrspnp.dip import DipNet
    nodes, c0, h, w, flat, x, t = _case(name)
    m = _mask(name, "pixel").cuda().reshape(-1).contiguous()
    net = DipNet(nodes, c0, h, w)
    net.stream.wait_stream(torch.cuda.current_stream())
    net.init_params(17)
    net.train_steps(x.cuda().contiguous(), t.cuda().contiguous(), m, 5, lr=0.01, use_graph=use_graph)
    torch.cuda.synchronize()
    return net.params.clone(), net.output().clone()


@pytest.mark.parametrize("name", ["golden", "ragged"])
def test_deterministic_and_graph_replay_equals_eager(L, name):
    p1, o1 = _train5(name, False)
    p2, o2 = _train5(name, False)
    assert torch.equal(p1, p2) and torch.equal(o1, o2)
    pg, og = _train5(name, True)
    assert torch.equal(p1, pg) and torch.equal(o1, og)
    assert bool(torch.isfinite(p1).all()) and bool(torch.isfinite(o1).all())


# ---- 4. one Adam step ---------------------------------------------------------------------------------
def test_one_adam_step_moves_by_lr_sign(L):
    """From the golden state one Adam step moves a parameter by -lr sign(g) (g / (|g| + eps) at step 1)
    wherever |g| is above the gradient's error bound of test_net_step0: per parameter tensor
    max(1e-4, twice the fp32-torch error) of ||g||, below which an element's sign is not determined."""
    from lrspnp.dip import DipNet
    nodes, c0, h, w, flat, x, t = _case("golden")
    m = _mask("golden", "pixel")
    ref = _reference("golden", "pixel")
    g32, g64 = ref[torch.float32][2], ref[torch.float64][2]
    lr = 0.01
    net = DipNet(nodes, c0, h, w)
    net.params.copy_(flat.cuda())
    net.reset_optimizer()
    net.train_steps(x.cuda().contiguous(), t.cuda().contiguous(), m.cuda().contiguous(), 1, lr=lr)
    torch.cuda.synchronize()
    delta = net.params.cpu().double() - flat.double()
    offs, _ = R.param_offsets(nodes, c0)
    checked = 0
    for i in range(len(nodes)):
        for j in (0, 2, 3):
            r = R.views(g64, nodes, i, offs, c0)[j]
            if r is None:
                continue
            f, d, p0 = (R.views(v, nodes, i, offs, c0)[j] for v in (g32.double(), delta, flat.double()))
            tau = max(1e-4, 2 * rel(f, r)) * float(r.norm())
            sel = r.abs() > tau
            checked += int(sel.sum())
            # |delta| = lr |g| / (|g| + 1e-8) through about ten float32 roundings (each <= 6e-8 relative:
            # 1e-6 of lr), then the rounding of the updated float32 parameter
            tol = lr * (1e-8 / r.abs()[sel] + 1e-6) + 2.0 ** -23 * (p0.abs()[sel] + lr)
            assert bool(((d[sel] + lr * torch.sign(r[sel])).abs() <= tol).all()), (i, j)
    assert checked > flat.numel() // 2


# ---- 5. DipProx and the solver ------------------------------------------------------------------------
def _dp_cfg(**kw):
    from lrspnp.dip import DipConfig
    return DipConfig(net="decoder", decoder_channels=(16, 16), learning_rate=0.01, **kw)


def _image_problem(H, W, kind="pixel", seed=2):
    rng = np.random.default_rng(seed)
    t = torch.from_numpy(rng.uniform(0, 1, (8, H, W)).astype(np.float32)).cuda()
    if kind == "pixel":
        m = torch.from_numpy((rng.random((H, W)) > 0.25).astype(np.float32)).cuda()
    else:
        from lrspnp.data import stripe_mask
        m = torch.from_numpy(stripe_mask(H, W, 8, seed=seed)).cuda()
    return t, m


def test_dipprox_equals_a_net_driven_by_hand(L):
    from lrspnp.dip import DipNet, DipProx, deep_decoder_nodes
    dp = DipProx(8, 36, 36, _dp_cfg())
    x = dp.decoder_input
    assert not dp.framed and tuple(x.shape) == (16, 9, 9) and dp.net.in_shape == (16, 9, 9)
    assert float(x.min()) >= 0.0 and float(x.max()) < 0.1 and float(x.std()) > 0.01
    t, m = _image_problem(36, 36)
    got = dp.run(t, None, m, seed=3, num_iter=4, early_stop=False).clone()
    torch.cuda.synchronize()
    assert dp.decoder_input is x and dp.last_steps == 4
    # the input argument is ignored for this net
    again = dp.run(t, torch.zeros(8, 36, 36, device="cuda"), m, seed=3, num_iter=4, early_stop=False)
    torch.cuda.synchronize()
    assert torch.equal(again, got)
    net = DipNet(deep_decoder_nodes(16, 8, (16, 16)), 16, 9, 9)
    net.stream.wait_stream(torch.cuda.current_stream())
    net.init_params(3)
    net.train_steps(x, t, m.reshape(-1), 4, lr=0.01)
    torch.cuda.synchronize()
    assert torch.equal(got, net.output()) and torch.equal(dp.net.params, net.params)
    assert dp.net.last_loss() == net.last_loss()
    # a second DipProx draws the same input
    assert torch.equal(DipProx(8, 36, 36, _dp_cfg()).decoder_input, x)


@pytest.mark.parametrize("kind", ["pixel", "band"])
def test_dipprox_framed_equals_a_net_framed_by_hand(L, kind):
    """38 x 45 trains inside the 40 x 48 frame at (1, 1): the target reflected, the mask 0 on the frame, the
    input (noise) not framed; the loss mean over the image alone; dL/dz of the head exactly 0 on the frame."""
    from lrspnp.dip import DipNet, DipProx, deep_decoder_nodes
    H, W, Hf, Wf, top, left = 38, 45, 40, 48, 1, 1
    nodes = deep_decoder_nodes(16, 8, (16, 16))
    dp = DipProx(8, H, W, _dp_cfg())
    assert dp.framed and (dp.Hf, dp.Wf, dp.top, dp.left) == (Hf, Wf, top, left)
    assert tuple(dp.decoder_input.shape) == (16, 10, 12) and dp.net.frame == (top, left, H, W)
    t, m = _image_problem(H, W, kind)
    got = dp.run(t, None, m, seed=5, num_iter=3, early_stop=False).clone()
    torch.cuda.synchronize()
    assert tuple(got.shape) == (8, H, W)
    tf = F.pad(t[None], (left, Wf - W - left, top, Hf - H - top), mode="reflect")[0].contiguous()
    mf = torch.zeros((m.numel() // (H * W), Hf, Wf), device="cuda")
    mf[:, top:top + H, left:left + W] = m.reshape(-1, H, W)
    mf = mf.reshape(-1) if kind == "pixel" else mf
    net = DipNet(nodes, 16, 10, 12)
    net.set_frame(top, left, H, W)
    net.stream.wait_stream(torch.cuda.current_stream())
    net.init_params(5)
    torch.cuda.synchronize()
    flat0 = net.params.cpu().clone()
    net.train_steps(dp.decoder_input, tf, mf, 1, lr=0.01)
    torch.cuda.synchronize()
    # the first step's loss: the mean over the image's 8 H W elements (1e-5: the output's tolerance)
    want = float(R.loss_fn(R.forward(flat0.double(), nodes, dp.decoder_input.cpu().double()), tf.cpu().double(),
                           mf.cpu().double(), n_mean=8 * H * W))
    assert abs(net.last_loss() - want) < 1e-5 * want
    gz = net.node_buffer(len(nodes) - 1, 2)
    frame = torch.ones(Hf, Wf, dtype=torch.bool, device="cuda")
    frame[top:top + H, left:left + W] = False
    assert bool((gz[:, frame] == 0).all()) and float(gz.abs().max()) > 0
    net.train_steps(dp.decoder_input, tf, mf, 2, lr=0.01)
    torch.cuda.synchronize()
    assert torch.equal(got, net.output()[:, top:top + H, left:left + W])
    assert torch.equal(dp.net.params, net.params) and dp.net.last_loss() == net.last_loss()


def test_dipprox_early_stopping_on_the_crops(L):
    """With early stopping on, the ring holds the cropped outputs and the device state is the one
    lrs_es_update_f32 reaches when fed those crops one by one."""
    from lrspnp.dip import DipNet, DipProx, EarlyStopper, EsState, deep_decoder_nodes
    H, W, Hf, Wf, top, left = 38, 45, 40, 48, 1, 1
    N, size, patience = 8 * H * W, 3, 2
    dp = DipProx(8, H, W, _dp_cfg(num_iter=9, es_size=size, patience=patience))
    t, m = _image_problem(H, W)
    got = dp.run(t, None, m, seed=1).clone()
    torch.cuda.synchronize()
    k = dp.last_steps
    assert size <= k <= 9 and tuple(got.shape) == (8, H, W)
    tf = F.pad(t[None], (left, Wf - W - left, top, Hf - H - top), mode="reflect")[0].contiguous()
    mf = torch.zeros((Hf, Wf), device="cuda")
    mf[top:top + H, left:left + W] = m
    mf = mf.reshape(-1)
    net = DipNet(deep_decoder_nodes(16, 8, (16, 16)), 16, 10, 12)
    net.set_frame(top, left, H, W)
    net.stream.wait_stream(torch.cuda.current_stream())
    net.init_params(1)
    es, ref = EarlyStopper(N, size, patience), EarlyStopper(N, size, patience)
    crops = []
    for i in range(k):
        net.train_steps(dp.decoder_input, tf, mf, 1, lr=0.01, es=es)
        torch.cuda.synchronize()
        cr = net.output()[:, top:top + H, left:left + W].contiguous()
        crops.append(cr.clone())
        assert torch.equal(es.slot_of(i).view(8, H, W), cr), i
        assert L.lrs_es_update_f32(P(cr), N, P(ref.ring), P(ref.state), S()) == 0
    torch.cuda.synchronize()
    a, b, c = dp.es.read(dp.net.stream), ref.read(), es.read(net.stream)
    assert a.count == k
    assert bytes(a) == bytes(b) == bytes(c), [(n, getattr(a, n), getattr(b, n)) for n, _ in EsState._fields_]
    assert torch.equal(dp.es.ring[:size * N], ref.ring[:size * N])
    epoch = dp.last_stop_epoch if dp.last_stop_epoch is not None else k - 1
    assert torch.equal(got, crops[epoch])


def test_solver_runs_the_decoder(L):
    """LrsPnP with dip_decoder on a 36 x 36 x 8 cube (bb = 8): two outer iterations; U is the direct
    DipProx.run on the same tensors and seed, bit for bit."""
    from lrspnp import LrsPnP, LrsPnPConfig, ops
    from lrspnp.data import mask_matrix, synthetic_cube, synthetic_dictionary, unfold
    H = W = 36
    B = 8
    obs, _, _ = synthetic_cube(H, W, B, seed=3)
    pix = (np.random.default_rng(0).random((H, W)) > 0.2).astype(np.float32)
    M = mask_matrix(pix, B)
    cfg = LrsPnPConfig.dip_decoder(bb=8, sliding=8, Nit=10, dip_seed=9, dip=_dp_cfg(num_iter=3, early_stop=False))
    s = LrsPnP(unfold(obs) * M, M, synthetic_dictionary(64, 256, 0), cfg, image_shape=(H, W))
    assert not s.framed and s.dip_in is None and s.dip.net.in_shape == (16, 9, 9)
    s.step()
    s.step()
    torch.cuda.synchronize()
    U = s.U.clone()
    assert tuple(U.shape) == (H * W, B) and bool(torch.isfinite(U).all())
    assert s.dip_steps == [(3, None), (3, None)]
    img = s.dip.run(s.dip_target.clone(), None, s.dip_mask, seed=9 + 1, early_stop=False)   # the second iteration's seed
    direct = ops.image_to_unfolded(img.contiguous(), H, W)
    torch.cuda.synchronize()
    assert torch.equal(U, direct)


def test_training_lowers_the_masked_loss(L):
    """From the golden state, the masked loss at step 100 (Adam, lr 0.01) is below the step-0 loss -- the
    condition tests/test_decoder_host.py::test_restatement_trains confirms for the restatement."""
    from lrspnp.dip import DipNet
    nodes, c0, h, w, flat, x, t = _case("golden")
    m = _mask("golden", "pixel").cuda().contiguous()
    net = DipNet(nodes, c0, h, w)
    net.params.copy_(flat.cuda())
    net.reset_optimizer()
    xd, td = x.cuda().contiguous(), t.cuda().contiguous()
    net.train_steps(xd, td, m, 1, lr=0.01)
    loss0 = net.last_loss()
    net.train_steps(xd, td, m, 100, lr=0.01)
    loss100 = net.last_loss()
    print("loss", loss0, loss100)
    assert abs(loss0 - float(_golden()["loss64"])) < 1e-6 * loss0
    assert np.isfinite(loss100) and loss100 < loss0


# ---- 6. the nn.Module drop-in -------------------------------------------------------------------------
def test_decodernw_module_step_vs_reference(L):
    from lrspnp.nn import decodernw
    g = _golden()
    nodes, c0, h, w, flat, x, t = _case("golden")
    net = decodernw(num_output_channels=8, num_channels_up=[16, 16]).cuda()
    net.load_flat(flat)
    params = list(net.parameters())
    assert sum(p.numel() for p in params) == flat.numel()
    assert [tuple(p.shape) for p in params[:3]] == [(16, 16, 1, 1), (16,), (16,)]
    opt = torch.optim.Adam(net.parameters(), 0.01)
    mse = torch.nn.MSELoss()
    X, T = x[None].cuda(), t[None].cuda()
    Mk = torch.from_numpy(g["mask"])[None, None].cuda()
    opt.zero_grad()
    out = net(X)
    assert out.shape == (1, 8, 36, 36)
    assert rel(out.detach()[0], g["out64"]) < 1e-5
    loss = mse(out * Mk, T * Mk)
    assert abs(float(loss.detach()) - float(g["loss64"])) < 1e-6 * float(g["loss64"])
    loss.backward()
    gflat = torch.cat([p.grad.reshape(-1).cpu() for p in params])
    _check_grads(nodes, c0, gflat, _reference("golden", "pixel"))
    before = net._flat.cpu().clone()
    opt.step()
    torch.cuda.synchronize()
    assert not torch.equal(net._flat.cpu(), before)
    out2 = net(X)
    assert bool(torch.isfinite(out2).all()) and rel(out2.detach(), out.detach()) > 1e-4
    # the activations the reference offers
    lre = decodernw(num_output_channels=8, num_channels_up=[16, 16], act_fun=torch.nn.LeakyReLU(0.2, inplace=True),
                    upsample_mode="none")
    assert lre(X).shape == (1, 8, 9, 9)

"""Host side of the Deep Decoder low-rank prox (no GPU): the DECODE node in lrs_dipnet_create, the
builder and the frame helpers, the plain-torch restatement (tests/decoder_ref.py) against the reference
module's own arithmetic (tests/golden/decoder_golden.npz: include/decoder.py decodernw run by torch on the
CPU in float32 and float64), and the arguments lrspnp.nn.decodernw refuses.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decoder_ref as R  # noqa: E402

from lrspnp import _lib  # noqa: E402
from lrspnp import dip as D  # noqa: E402

E_INVALID, E_UNSUPPORTED = -1, -2


def create(nodes, C, H, W):
    """(status, handle) of lrs_dipnet_create: host only."""
    L = _lib.lib()
    arr = (D.DipNode * len(nodes))(*nodes)
    h = ctypes.c_void_p()
    opts = _lib.dip_opts()
    rc = L.lrs_dipnet_create(arr, len(nodes), C, H, W, ctypes.byref(opts), ctypes.byref(h))
    return rc, h


def test_node_struct_size_unchanged():
    assert ctypes.sizeof(D.DipNode) == 52   # 13 int32: existing callers build it positionally


def test_create_accepts_decoder_and_reports_layout():
    L = _lib.lib()
    nodes = D.deep_decoder_nodes(16, 8, (16, 16))
    assert len(nodes) == 4 and [n.upsample for n in nodes] == [2, 2, 0, 0]
    assert [n.act for n in nodes] == [D.ACT_RELU] * 3 + [D.ACT_SIGMOID] and [n.bn for n in nodes] == [1, 1, 1, 0]
    rc, h = create(nodes, 16, 9, 9)
    assert rc == 0
    try:
        c, ho, wo = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        assert L.lrs_dipnet_out_shape(h, ctypes.byref(c), ctypes.byref(ho), ctypes.byref(wo)) == 0
        assert (c.value, ho.value, wo.value) == (8, 36, 36)
        shapes = []
        for i in range(4):
            L.lrs_dipnet_node_shape(h, i, ctypes.byref(c), ctypes.byref(ho), ctypes.byref(wo))
            shapes.append((c.value, ho.value, wo.value))
        assert shapes == [(16, 18, 18), (16, 36, 36), (16, 36, 36), (8, 36, 36)]
        # per stage: W [16][16], gamma, beta; the head: W [8][16]; no bias anywhere
        want, p = [], 0
        for i in range(3):
            want.append((p, -1, p + 256, p + 272))
            p += 288
        want.append((p, -1, -1, -1))
        p += 128
        got = []
        for i in range(4):
            o = [ctypes.c_int64() for _ in range(4)]
            assert L.lrs_dipnet_param_offsets(h, i, *[ctypes.byref(v) for v in o]) == 0
            got.append(tuple(v.value for v in o))
        assert got == want
        assert L.lrs_dipnet_num_params(h) == p == 992
        assert L.lrs_dipnet_num_bnstats(h) == 2 * 16 * 3
        assert L.lrs_dipnet_workspace(h) > 0
        offs, total = R.param_offsets(nodes, 16)   # the restatement's layout is the engine's
        assert offs == want and total == p
    finally:
        L.lrs_dipnet_destroy(h)


def _decode(**kw):
    d = dict(kind=D.NODE_DECODE, in0=0, in1=0, cout=8, k=1, stride=1, pad=0, pad_mode=0, upsample=D.UP_BILINEAR,
             bn=D.BN_PLAIN, act=D.ACT_RELU, sn=0, winit=0)
    d.update(kw)
    return D.DipNode(*[d[n] for n, _ in D.DipNode._fields_])


@pytest.mark.parametrize("node, status", [
    (_decode(k=3), E_UNSUPPORTED),
    (_decode(stride=2), E_UNSUPPORTED),
    (_decode(pad=1), E_UNSUPPORTED),
    (_decode(sn=1), E_UNSUPPORTED),
    (_decode(bn=D.BN_LIP), E_UNSUPPORTED),
    (_decode(upsample=D.UP_NEAREST), E_UNSUPPORTED),
    (_decode(act=D.ACT_SIGMOID), E_INVALID),                              # sigmoid with upsampling (and BN)
    (_decode(act=D.ACT_SIGMOID, bn=D.BN_NONE), E_INVALID),                # sigmoid with upsampling
    (_decode(act=D.ACT_SIGMOID, upsample=0), E_INVALID),                  # sigmoid with BN
    (_decode(kind=D.NODE_CONV, upsample=0, bn=D.BN_NONE), E_INVALID),     # ReLU on a CONV node
    (_decode(kind=D.NODE_BN, upsample=0), E_INVALID),                     # ReLU on a BN node
    (_decode(kind=D.NODE_CONV, act=D.ACT_LRELU, bn=D.BN_NONE), E_INVALID),   # bilinear upsampling on a CONV node
    (_decode(kind=D.NODE_CONCAT, act=D.ACT_NONE, bn=D.BN_NONE), E_INVALID),  # ... and on a CONCAT node
])
def test_create_refuses(node, status):
    rc, h = create([node], 4, 6, 6)
    if rc == 0:
        _lib.lib().lrs_dipnet_destroy(h)
    assert rc == status


def test_create_still_accepts_what_it_did():
    """The head form (sigmoid, no BN, no upsampling), LeakyReLU stages, and a CONV with nearest upsampling."""
    for nodes in ([_decode(act=D.ACT_SIGMOID, upsample=0, bn=D.BN_NONE)], [_decode(act=D.ACT_LRELU)],
                  [_decode(act=D.ACT_NONE, bn=D.BN_NONE)],
                  [_decode(kind=D.NODE_CONV, act=D.ACT_LRELU, upsample=D.UP_NEAREST, bn=D.BN_NONE)]):
        rc, h = create(nodes, 4, 6, 6)
        assert rc == 0
        _lib.lib().lrs_dipnet_destroy(h)


def test_builder_follows_decodernw():
    n = D.deep_decoder_nodes(32, 5, (32, 24, 16), act="lrelu", need_sigmoid=False, bn=False)
    assert [d.cout for d in n] == [24, 16, 16, 16, 5]              # num_channels_up + [last, last], then the head
    assert [d.upsample for d in n] == [2, 2, 2, 0, 0]
    assert all(d.kind == D.NODE_DECODE and d.k == 1 and d.bn == 0 for d in n)
    assert [d.act for d in n] == [D.ACT_LRELU] * 4 + [D.ACT_NONE]
    assert [d.in0 for d in n] == list(range(5))
    assert D.decoder_scale(n) == 8 and D.decoder_scale(D.skip_nodes(4, 4)) is None
    with pytest.raises(ValueError):
        D.deep_decoder_nodes(8, 5, (32, 24))       # the input has channels[0] channels


def test_frame_helpers_for_the_decoder():
    nodes = D.deep_decoder_nodes(16, 8, (16, 16))
    assert D.net_out_hw(nodes, 9, 9) == (36, 36) and D.net_out_hw(nodes, 10, 12) == (40, 48)
    assert D.frame_for(nodes, 36, 36) == (36, 36, 0, 0)
    assert D.frame_for(nodes, 38, 45) == (40, 48, 1, 1)
    assert D.out_size(9, 7, 1, 1, 0, D.UP_BILINEAR) == (18, 14)
    # the image nets' frames are what they were
    assert D.frame_for(D.lipschitz_unet_nodes(4, 4, 8), 40, 40) == (52, 52, 6, 6)


def test_up2_restatement_is_torch_bilinear():
    g = torch.Generator().manual_seed(3)
    for shape in ((1, 1, 1), (3, 1, 5), (5, 2, 3), (7, 17, 33)):
        x = torch.randn(shape, generator=g, dtype=torch.float64)
        want = torch.nn.functional.interpolate(x[None], scale_factor=2, mode="bilinear", align_corners=False)[0]
        assert torch.allclose(R.up2_bilinear(x), want, rtol=0, atol=1e-14)


@pytest.mark.parametrize("tag, dtype, tol_out, tol_loss, tol_grad", [
    ("32", torch.float32, 1e-6, 1e-6, 1e-5), ("64", torch.float64, 1e-12, 1e-12, 1e-12)])
def test_restatement_reproduces_the_reference_module(golden, tag, dtype, tol_out, tol_loss, tol_grad):
    g = golden("decoder_golden.npz")
    nodes = D.deep_decoder_nodes(16, 8, tuple(int(c) for c in g["channels"]))
    flat = R.flat_from_golden(g, dtype)
    x, t, m = (torch.from_numpy(g[k]).to(dtype) for k in ("x", "target", "mask"))
    out, loss, grad = R.step0(flat, nodes, x, t, m)
    ref = torch.from_numpy(g["out" + tag])
    assert out.shape == (8, 36, 36)
    assert float((out - ref).norm() / ref.norm()) < tol_out
    assert abs(float(loss) - float(g["loss" + tag])) < tol_loss * float(g["loss" + tag])
    off = 0
    for name in g["param_names"]:
        gr = torch.from_numpy(g[f"g{tag}/{name}"]).reshape(-1)
        mine = grad[off:off + gr.numel()]
        off += gr.numel()
        assert float((mine - gr).norm() / gr.norm()) < tol_grad, name
    assert off == grad.numel()


def test_restatement_trains():
    """The condition the GPU training-sanity test asserts, confirmed on the restatement: at the golden
    state the masked loss after 100 Adam steps at lr 0.01 is below the step-0 loss."""
    g = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decoder_golden.npz")))
    nodes = D.deep_decoder_nodes(16, 8, (16, 16))
    x, t, m = (torch.from_numpy(g[k]) for k in ("x", "target", "mask"))
    losses, _ = R.train(R.flat_from_golden(g), nodes, x, t, m, steps=101, lr=0.01)
    assert losses[100] < losses[0]


def test_solver_config():
    from lrspnp import LrsPnPConfig
    from lrspnp._lib import LrsError
    c = LrsPnPConfig.dip_decoder(bb=8, sliding=8)
    assert c.lowrank == "dip" and c.dip.net == "decoder" and c.dip.learning_rate == 0.01 and not c.dip.early_stop
    assert c.dip.decoder_channels == (128, 128) and c.dip.decoder_input_scale == 0.1
    with pytest.raises(LrsError):
        LrsPnPConfig.dip_decoder(dip=D.DipConfig(net="skip"))
    assert [n.cout for n in D.dip_nodes(D.DipConfig(net="decoder", decoder_channels=(16, 12)), 8)] == [12, 12, 12, 8]


@pytest.mark.parametrize("kw, word", [
    (dict(filter_size_up=3), "filter_size_up"),
    (dict(filter_size_up=[1, 3, 1, 1]), "filter_size_up"),
    (dict(upsample_mode="nearest"), "upsample_mode"),
    (dict(act_fun=torch.nn.Tanh()), "act_fun"),
    (dict(act_fun=torch.nn.LeakyReLU(0.1)), "act_fun"),
    (dict(bn_before_act=True), "bn_before_act"),
    (dict(bn_affine=False), "bn_affine"),
    (dict(upsample_first=False), "upsample_first"),
])
def test_decodernw_refuses_unsupported_arguments(kw, word):
    """Each refusal names its argument, before any engine (or device) is touched."""
    from lrspnp.nn import decodernw
    with pytest.raises(NotImplementedError, match=word):
        decodernw(num_output_channels=8, num_channels_up=[16, 16], **kw)


def test_shim_maps_include_decoder():
    from lrspnp import shim
    assert shim._TARGETS["include.decoder"] == ("lrspnp.nn", ["decodernw"])

"""One sha256 per output tensor of the DIP conv products, for bitwise A/B of two builds (LRSPNP_LIB).

    python tools/conv_digest.py > new.txt
    LRSPNP_LIB=.../liblrspnp_hip_parent.so python tools/conv_digest.py > parent.txt     # then diff

Primitive ABI: every conv case of tests/test_gpu_dip.py (CONV_CASES) through lrs_conv2d_fwd_f32 and
lrs_conv2d_bwd_f32 with a col buffer (split-bf16 and f32) and through lrs_conv2d_fwd_f32 and
lrs_conv2d_bwd_x_f32 without one (upsample_dgrad 0 and 1): y, gw, gx.  Engine: three training steps
from seed 0 on the 36 x 36 x 7 and 66 x 66 x 7 U-Nets and the 36 x 36 x 128 skip net, each with the
default options, with upsample_dgrad = 1 and with precision = LRS_DIP_F32 (output, parameters,
gradients): implicit and small-map paths, split-K with S > 1 and S = 1, the parity-class convs, and
on the 66^2 net maps that are no multiple of 4.  The same three steps on two Deep Decoders and their
variants (no BatchNorm, no sigmoid, f32, a per-band mask, a frame), and one forward + backward on each.
Then every form of the training step (StepPlan, dipnet_plan.h) the nets above leave out: the overlapped
sigma (a 196 x 196 x 7 U-Net of hidden width OVERLAP_HIDDEN, eager and as a replayed graph), the loss head
demoted from k_pw's epilogue by a misaligned mask, a net whose last node is a BatchNorm (the generic
head), early stopping with and without a frame (the ring and the state too), and a stand-alone forward +
backward on a U-Net.  (The 36^2 U-Net above has the head in k_pw's epilogue, the 66^2 one k_mse_head.)
"""
import ctypes
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "lrs-pnp-dip_amd"))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from lrspnp import _lib  # noqa: E402
from lrspnp.dip import (ACT_NONE, BN_NONE, BN_PLAIN, NODE_BN, DipNet, DipNode, EarlyStopper, conv_node,  # noqa: E402
                        deep_decoder_nodes, lipschitz_unet_nodes, skip_nodes)
from test_gpu_dip import CONV_CASES, P, S  # noqa: E402


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


L = _lib.device_lib()
for ci, case in enumerate(CONV_CASES):
    cin, cout, H, W, k, stride, pad, pm, up = case
    g = torch.Generator().manual_seed(ci)
    x = torch.randn(cin, H, W, generator=g).cuda()
    w = (torch.randn(cout, cin, k, k, generator=g) / np.sqrt(cin * k * k)).cuda()
    b = (torch.randn(cout, generator=g) * 0.1).cuda()
    Ho, Wo = ctypes.c_int(), ctypes.c_int()
    assert L.lrs_conv2d_out_size(H, W, k, stride, pad, up, ctypes.byref(Ho), ctypes.byref(Wo)) == 0
    gy = torch.randn(cout, Ho.value, Wo.value, generator=g).cuda()
    div = torch.tensor([1.7], device="cuda")
    ncol = L.lrs_conv2d_col_size(cin, H, W, k, stride, pad, up)
    # (explicit, precision, upsample_dgrad)
    for explicit, prec, ud in ((1, 1, 0), (1, 0, 0), (0, 1, 0), (0, 1, 1)):
        opts = ctypes.byref(_lib.dip_opts(prec, ud))
        nws = L.lrs_conv2d_workspace(cin, H, W, cout, k, stride, pad, up, opts)
        ws = torch.zeros(nws // 4 + 1, device="cuda")
        col = torch.zeros(max(ncol, 1), device="cuda")
        y = torch.full((cout, Ho.value, Wo.value), float("nan"), device="cuda")
        gw, gx = torch.full_like(w, float("nan")), torch.full_like(x, float("nan"))
        geo = (cin, H, W, cout, k, stride, pad, pm, up)
        rc = L.lrs_conv2d_fwd_f32(P(x), cin, H, W, P(w), P(b), cout, k, stride, pad, pm, up,
                                  P(col) if explicit and ncol else None, P(y), opts, P(ws), nws, S())
        if explicit:
            rc2 = L.lrs_conv2d_bwd_f32(P(gy), P(col) if ncol else P(x), P(w), P(div), *geo, P(gx), P(gw), opts, P(ws), nws,
                                       S())
        else:
            rc2 = L.lrs_conv2d_bwd_x_f32(P(gy), P(x), P(w), P(div), *geo, P(gx), P(gw), opts, P(ws), nws, S())
        torch.cuda.synchronize()
        tag = f"conv {ci} {'col' if explicit else 'implicit'} prec={prec} updgrad={ud} rc={rc},{rc2}"
        for name, t in (("y", y), ("gw", gw), ("gx", gx)):
            print(f"{tag} {name} {sha(t)}")

for name, nodes, bands, hw in (("unet36x7", lipschitz_unet_nodes(7, 7, 128), 7, 36),
                               ("unet66x7", lipschitz_unet_nodes(7, 7, 128), 7, 66),
                               ("skip36x128", skip_nodes(128, 128), 128, 36)):
    for oname, kw in (("default", {}), ("updgrad", {"upsample_dgrad": 1}), ("f32", {"precision": _lib.DIP_F32})):
        net = DipNet(nodes, bands, hw, hw, **kw)
        net.init_params(0)
        g = torch.Generator(device="cuda").manual_seed(0)
        x = torch.rand(bands, hw, hw, device="cuda", generator=g)
        Co, Ho, Wo = net.out_shape   # (a size that is no multiple of 4 comes out larger than it went in)
        t = torch.rand(Co, Ho, Wo, device="cuda", generator=g)
        m = (torch.rand(Ho, Wo, device="cuda", generator=g) > 0.2).float()
        net.train_steps(x, t, m, 3, use_graph=False)
        torch.cuda.synchronize()
        for k, v in (("output", net.output()), ("params", net.params), ("grads", net.grads), ("bnstats", net.bnstats)):
            print(f"net {name} {oname} {k} {sha(v)}")

# The Deep Decoder (DECODE nodes).  dec36x7: channels (128, 128), 9 x 9 -> 36 x 36 x 7: the 81- and 324-pixel
# stages on the dense GEMM, the 1296-pixel stage and the head on k_pw, the loss head in its epilogue.
# dec68x5: channels (16, 16), 17 x 17 -> 68 x 68 x 5: the odd width takes the scalar form of the x2 kernels,
# the 4624-pixel head is above the fused head's limit (k_mse_head).
# (name, channels, bands, input side, deep_decoder_nodes options, DipNet options, per-band mask, frame)
DEC36, DEC68 = ("dec36x7", (128, 128), 7, 9), ("dec68x5", (16, 16), 5, 17)
for (name, ch, bands, hw), oname, nkw, kw, cmask, frame in (
        (DEC36, "default", {}, {}, False, None),
        (DEC68, "default", {}, {}, False, None),
        (DEC36, "nobn-lrelu", {"bn": False, "act": "lrelu"}, {}, False, None),
        (DEC36, "nosigmoid", {"need_sigmoid": False}, {}, False, None),
        (DEC36, "f32", {}, {"precision": _lib.DIP_F32}, False, None),
        (DEC36, "bandmask", {}, {}, True, None),
        (DEC68, "frame", {}, {}, False, (2, 1, 64, 66))):
    net = DipNet(deep_decoder_nodes(ch[0], bands, ch, **nkw), ch[0], hw, hw, **kw)
    net.init_params(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand(ch[0], hw, hw, device="cuda", generator=g) * 0.1
    Co, Ho, Wo = net.out_shape
    t = torch.rand(Co, Ho, Wo, device="cuda", generator=g)
    m = (torch.rand((Co, Ho, Wo) if cmask else (Ho, Wo), device="cuda", generator=g) > 0.2).float()
    if frame:
        top, left, fh, fw = frame
        net.set_frame(*frame)
        inside = torch.zeros_like(m)
        inside[top:top + fh, left:left + fw] = 1.0
        m = m * inside
    net.train_steps(x, t, m, 3, use_graph=False)
    torch.cuda.synchronize()
    for k, v in (("output", net.output()), ("params", net.params), ("grads", net.grads), ("bnstats", net.bnstats)):
        print(f"net {name} {oname} {k} {sha(v)}")
    if oname == "default":   # forward + backward from a given dL/dout: the head's own activation backward
        gout = torch.randn(Co, Ho, Wo, device="cuda", generator=g)
        net.forward(x)
        net.backward(x, gout)
        torch.cuda.synchronize()
        print(f"net {name} fwdbwd grads {sha(net.grads)}")


# ---- the step's forms ----------------------------------------------------------------------------
# the narrowest U-Net that takes the overlapped sigma at 196^2 (k_sn_gram_head in a kernel trace); its
# first conv's map is 98^2, the smallest that does
OVERLAP_HIDDEN = 16


def step_case(tag, nodes, cin, hw, use_graph=False, shift_mask=False, frame=None, es=False, fwdbwd=False):
    net = DipNet(nodes, cin, hw, hw)
    net.init_params(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand(cin, hw, hw, device="cuda", generator=g)
    Co, Ho, Wo = net.out_shape
    t = torch.rand(Co, Ho, Wo, device="cuda", generator=g)
    m = (torch.rand(Ho, Wo, device="cuda", generator=g) > 0.2).float()
    if frame:
        top, left, fh, fw = frame
        net.set_frame(*frame)
        inside = torch.zeros_like(m)
        inside[top:top + fh, left:left + fw] = 1.0
        m = m * inside
    if shift_mask:   # the same mask one float into its storage: no longer 16-byte aligned
        store = torch.zeros(Ho * Wo + 1, device="cuda")
        store[1:] = m.flatten()
        m = store[1:].view(Ho, Wo)
        assert m.data_ptr() % 16 == 4
    stopper = EarlyStopper(Co * net.frame[2] * net.frame[3], size=2, patience=60) if es else None
    if fwdbwd:
        net.forward(x)
        net.backward(x, torch.randn(Co, Ho, Wo, device="cuda", generator=g))
    else:
        net.train_steps(x, t, m, 3, es=stopper, use_graph=use_graph)
    torch.cuda.synchronize()
    out = [("output", net.output()), ("params", net.params), ("grads", net.grads), ("bnstats", net.bnstats)]
    if es:
        out += [("es_ring", stopper.ring), ("es_state", stopper.state)]
    for k, v in out:
        print(f"step {tag} {k} {sha(v)}")


def bn_node(src):
    return DipNode(NODE_BN, src, 0, 0, 0, 0, 0, 0, 0, BN_PLAIN, ACT_NONE, 0, 0)


unet196 = lipschitz_unet_nodes(7, 7, OVERLAP_HIDDEN)
unet36 = lipschitz_unet_nodes(7, 7, 128)
step_case(f"overlap unet196x7h{OVERLAP_HIDDEN} eager", unet196, 7, 196)
step_case(f"overlap unet196x7h{OVERLAP_HIDDEN} graph", unet196, 7, 196, use_graph=True)
step_case("demoted unet36x7 mask+4B", unet36, 7, 36, shift_mask=True)
step_case("generic bn8x7", [bn_node(0)], 7, 8)
step_case("generic convbn8x7", [conv_node(0, 0, 8, 3, bn=BN_NONE, act=ACT_NONE, sn=0), bn_node(1)], 7, 8)
step_case("es unet36x7", unet36, 7, 36, es=True)
step_case("es unet36x7 frame", unet36, 7, 36, es=True, frame=(2, 1, 32, 34))
step_case("es unet36x7 graph", unet36, 7, 36, es=True, use_graph=True)
step_case("fwdbwd unet36x7", unet36, 7, 36, fwdbwd=True)

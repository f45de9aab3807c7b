"""Plain-torch restatement of the Deep Decoder as the engine runs it (LRS_NODE_DECODE chains), for tests.

Written from the stage's definition, not from the reference's module: per node
    z = W x  (1x1 conv, no bias)  ->  [bilinear x2, align_corners=False]  ->  act  ->  [BatchNorm, train mode]
with the parameters in the engine's flat layout (per node: W [cout][cin], then gamma, beta when the node has
BatchNorm).  The dtype follows the flat parameter tensor, so the same code is the fp32 and the fp64
reference.  Also the masked-MSE loss (optionally over a framed image) and the training loop with torch's
Adam.  oracle/dip_ref.py restates the CONV / BN / CONCAT nodes; it cannot express this one.
"""
from __future__ import annotations

import torch

NODE_DECODE = 3
ACT_NONE, ACT_LRELU, ACT_SIGMOID, ACT_RELU = 0, 1, 2, 3
BN_EPS = 1e-5


def node_dicts(nodes):
    return [n if isinstance(n, dict) else n.as_dict() for n in nodes]


def channels(nodes, c0):
    """Channel count of every tensor (tensor 0 = the input)."""
    ch = [int(c0)]
    for d in node_dicts(nodes):
        assert d["kind"] == NODE_DECODE, "decoder_ref restates DECODE nodes only"
        ch.append(int(d["cout"]))
    return ch


def param_offsets(nodes, c0):
    """[(w, b = -1, gamma, beta)] per node (floats into the flat buffer, -1 = absent) and the total."""
    ch, offs, p = channels(nodes, c0), [], 0
    for i, d in enumerate(node_dicts(nodes)):
        w = p
        p += ch[i + 1] * ch[d["in0"]]
        g = be = -1
        if d["bn"]:
            g, be = p, p + ch[i + 1]
            p += 2 * ch[i + 1]
        offs.append((w, -1, g, be))
    return offs, p


def views(flat, nodes, i, offs, c0):
    """(W [cout][cin], None, gamma | None, beta | None) of node i as views of flat."""
    ch, d = channels(nodes, c0), node_dicts(nodes)[i]
    w, _, g, be = offs[i]
    co, ci = ch[i + 1], ch[d["in0"]]
    return (flat[w:w + co * ci].view(co, ci), None, flat[g:g + co] if g >= 0 else None,
            flat[be:be + co] if be >= 0 else None)


def up2_bilinear(x):
    """(C, H, W) -> (C, 2H, 2W): output 2s + p takes 3/4 of source s and 1/4 of s - 1 (p = 0) or s + 1
    (p = 1), the neighbour's index clamped to the map (nn.Upsample(x2, bilinear, align_corners=False))."""
    def axis(t, dim):
        n = t.shape[dim]
        idx = torch.arange(n, device=t.device)
        lo = t.index_select(dim, (idx - 1).clamp(min=0))
        hi = t.index_select(dim, (idx + 1).clamp(max=n - 1))
        even, odd = 0.75 * t + 0.25 * lo, 0.75 * t + 0.25 * hi
        shape = list(t.shape)
        shape[dim] = 2 * n
        return torch.stack((even, odd), dim=dim + 1).reshape(shape)
    return axis(axis(x, 1), 2)


def act(x, a):
    if a == ACT_RELU:
        return torch.relu(x)
    if a == ACT_LRELU:
        return torch.nn.functional.leaky_relu(x, 0.2)
    if a == ACT_SIGMOID:
        return torch.sigmoid(x)
    return x


def forward(flat, nodes, x, keep=None):
    """Network output (C, H, W) for input x (c0, h, w); keep (a list) receives every node's output."""
    nd = node_dicts(nodes)
    offs, total = param_offsets(nodes, x.shape[0])
    assert flat.numel() == total, (flat.numel(), total)
    tensors = [x.to(flat.dtype)]
    for i, d in enumerate(nd):
        W, _, g, be = views(flat, nodes, i, offs, x.shape[0])
        t = torch.einsum("oc,chw->ohw", W, tensors[d["in0"]])
        if d["upsample"]:
            t = up2_bilinear(t)
        t = act(t, d["act"])
        if d["bn"]:   # training mode: batch statistics, biased variance
            m = t.mean(dim=(1, 2), keepdim=True)
            v = ((t - m) ** 2).mean(dim=(1, 2), keepdim=True)
            t = (t - m) / torch.sqrt(v + BN_EPS) * g.view(-1, 1, 1) + be.view(-1, 1, 1)
        tensors.append(t)
        if keep is not None:
            keep.append(t)
    return tensors[-1]


def loss_fn(out, target, mask=None, n_mean=None):
    """MSELoss(target * mask, out * mask): the mean over all C H W elements, or over n_mean (the image
    inside a frame, where the mask is 0 outside).  mask: None, (P,) / (H, W), or (C, H, W)."""
    C, H, W = out.shape
    if mask is None:
        m = torch.ones((), dtype=out.dtype, device=out.device)
    else:
        m = mask.to(out.dtype).reshape((1, H, W) if mask.numel() == H * W else (C, H, W))
    d = target.to(out.dtype) * m - out * m
    return (d * d).sum() / (out.numel() if n_mean is None else n_mean)


def step0(flat, nodes, x, target, mask=None, n_mean=None):
    """(output, loss, flat gradient) at the parameters flat, in flat's dtype."""
    p = flat.detach().clone().requires_grad_(True)
    out = forward(p, nodes, x)
    loss = loss_fn(out, target, mask, n_mean)
    loss.backward()
    return out.detach(), loss.detach(), p.grad.detach()


def train(flat, nodes, x, target, mask=None, steps=1, lr=0.01, n_mean=None):
    """steps of forward, masked MSE, backward, torch.optim.Adam(lr) (include/fit.py's loop); returns the
    per-step losses (before each update) and the final flat parameters."""
    p = flat.detach().clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = loss_fn(forward(p, nodes, x), target, mask, n_mean)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses, p.detach()


def flat_from_golden(gold, dtype=torch.float32):
    """The reference module's parameters (a decoder_golden.npz dict) in the engine's flat order: the
    module's named_parameters() order -- per stage the conv weight, then the BatchNorm weight and bias."""
    parts = [torch.from_numpy(gold["sd/" + str(n)]).reshape(-1) for n in gold["param_names"]]
    return torch.cat(parts).to(dtype)

"""Generate tests/golden/decoder_golden.npz from the reference's own Deep Decoder.

    python tests/golden/gen_decoder_golden.py /path/to/LRS-PnP-DIP        (or LRSPNP_REFERENCE=...)

Imports decodernw from the reference checkout's include/decoder.py and runs it on the CPU, in float32 and
in float64 from the same parameters: num_channels_up=[16, 16], 8 output bands, a seeded 16 x 9 x 9 input
(uniform on [0, 0.1), as include/fit.py draws it), giving an 8 x 36 x 36 output.  The convs keep the module's
own (torch-seeded) initial weights; the BatchNorm weights and biases are set to seeded non-trivial values so
that their gradients are exercised.  Stored (data only): the state dict ("sd/<name>", float32) and the
parameter names in named_parameters() order, the input, a seeded target and pixel mask, and per dtype
the output, the masked loss MSELoss(out * mask, target * mask) (include/fit.py) and every parameter's
gradient at step 0 ("g64/<name>", "g32/<name>").
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 4321
CHANNELS, BANDS, SIDE = [16, 16], 8, 9


def problem(seed=SEED, c0=CHANNELS[0], bands=BANDS, side=SIDE, scale=2 ** len(CHANNELS)):
    """Seeded input (c0, side, side) on [0, 0.1), target (bands, H, W) in (0, 1) and pixel mask (H, W)."""
    rng = np.random.default_rng(seed)
    H = side * scale
    x = (rng.uniform(0, 1, (c0, side, side)) * 0.1).astype(np.float32)
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, H), indexing="ij")
    ph = rng.uniform(0, 2 * np.pi, (bands, 1, 1))
    fr = rng.uniform(1, 4, (bands, 1, 1))
    target = 0.5 + 0.35 * np.sin(2 * np.pi * fr * (yy + 0.5 * xx)[None] + ph) + 0.05 * rng.standard_normal((bands, H, H))
    mask = (rng.uniform(0, 1, (H, H)) > 0.3).astype(np.float32)
    return x, np.clip(target, 0.0, 1.0).astype(np.float32), mask


def main():
    ref = os.environ.get("LRSPNP_REFERENCE") or (sys.argv[1] if len(sys.argv) > 1 else None)
    if not ref:
        sys.exit(__doc__)
    sys.path.insert(0, ref)
    from include.decoder import decodernw   # the reference module itself

    torch.manual_seed(SEED)
    net = decodernw(num_output_channels=BANDS, num_channels_up=list(CHANNELS))
    rng = np.random.default_rng(SEED + 1)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if p.dim() == 1:   # BatchNorm weight / bias
                u = torch.from_numpy(rng.uniform(-1, 1, p.shape).astype(np.float32))
                p.copy_(1.0 + 0.25 * u if name.endswith("weight") else 0.1 * u)
    names = [n for n, _ in net.named_parameters()]
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    x, target, mask = problem()
    out = {"param_names": np.array(names), "x": x, "target": target, "mask": mask, "seed": np.int64(SEED),
           "channels": np.array(CHANNELS, np.int64)}
    for k, v in sd.items():
        out["sd/" + k] = v.numpy()
    mse = torch.nn.MSELoss()
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        m = decodernw(num_output_channels=BANDS, num_channels_up=list(CHANNELS)).to(dt)
        m.load_state_dict({k: v.to(dt) if v.is_floating_point() else v for k, v in sd.items()})
        m.train()
        X, T = torch.from_numpy(x).to(dt)[None], torch.from_numpy(target).to(dt)[None]
        M = torch.from_numpy(mask).to(dt)[None, None]
        o = m(X)
        loss = mse(o * M, T * M)
        loss.backward()
        out["out" + tag] = o.detach()[0].numpy()
        out["loss" + tag] = np.float64(loss.detach())
        for n, p in m.named_parameters():
            out[f"g{tag}/{n}"] = p.grad.numpy()
        print(tag, "loss", float(loss.detach()), "out", tuple(o.shape))
    path = os.path.join(HERE, "decoder_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

"""Time of one spectral-NLM call on the cube (ops.nlmcube, lrs_nlmcube_f32) by device events: median over rounds
of several calls, per cube and (patch_size, patch_distance), with the rates of the work DESIGN §13 counts (the
pixel-distance and weighted-sum FLOP, the compulsory bytes); then the outer iteration of the 200x200x198 cube
(BASELINE configs[1]: 8x8 blocks, 80 sparse-coding iterations) with lowrank="svt", "tv" and "nlm", for context.

    python tools/nlmcube_time.py [--cubes 196x196x198 200x200x198] [--params 7,2 3,3] [--calls 10] [--rounds 7]
                                 [--no-solver] [--out profiles/nlmcube/nlmcube_time.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "lrs-pnp-dip_amd"))
import torch  # noqa: E402
from lrspnp import LrsPnP, LrsPnPConfig, NlmCubeConfig, TvProxConfig, ops  # noqa: E402

HBM = 6.3e12   # achievable HBM rate, bytes/s
TILE = 8       # the kernel's spatial tile edge (csrc/nlmcube.hip)


def call_work(H, W, B, ps, pd):
    """(useful FLOP, FLOP the tiles execute, compulsory bytes, bytes the tiles load and store) of one call.
    Useful: 2 P B T for the pixel distances (each d once per pixel and offset; the box sums reuse them) and
    2 P B T for the weighted sums, T = (2 pd + 1)^2.  Executed: a tile forms d on its (8 + 2 rp)^2 extended
    positions.  Compulsory: X, L2 in and U out, once.  Loaded: the halo of (8 + 2 (rp + pd))^2 pixels for the
    distances and of (8 + 2 pd)^2 for the sums, per 64 pixels, X and L2 each."""
    P, T, rp = H * W, (2 * pd + 1) ** 2, ps // 2
    tiles = -(-H // TILE) * -(-W // TILE)
    useful = 4 * P * B * T
    executed = 2 * tiles * (TILE + 2 * rp) ** 2 * B * T + 2 * tiles * TILE * TILE * B * T
    compulsory = 4 * P * B * 3
    moved = 4 * B * (2 * tiles * ((TILE + 2 * (rp + pd)) ** 2 + (TILE + 2 * pd) ** 2) + P)
    return useful, executed, compulsory, moved


def median_ms(fn, calls, rounds):
    fn()
    torch.cuda.synchronize()
    res = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        res.append(e0.elapsed_time(e1) / calls)
    return statistics.median(res), min(res), max(res)


def time_cube(H, W, B, a):
    g = torch.Generator(device="cuda").manual_seed(0)
    X = torch.rand(H * W, B, device="cuda", generator=g)
    L2 = (torch.rand(H * W, B, device="cuda", generator=g) - 0.5) * 0.1
    U = torch.empty_like(X)
    rows = []
    for ps, pd in a.params:
        ws = ops.nlmcube_workspace(H, W, B, ps, pd, "cuda")
        med, lo, hi = median_ms(lambda: ops.nlmcube(X, L2, 0.5, H, W, ws, U=U, patch_size=ps, patch_distance=pd, h=0.2),
                                a.calls, a.rounds)
        useful, executed, compulsory, moved = call_work(H, W, B, ps, pd)
        s = med * 1e-3
        rows.append(dict(cube=f"{H}x{W}x{B}", patch_size=ps, patch_distance=pd, ms=med, ms_min=lo, ms_max=hi,
                         useful_flop=useful, executed_flop=executed, compulsory_bytes=compulsory, moved_bytes=moved,
                         useful_flop_per_s=useful / s, moved_bytes_per_s=moved / s,
                         compulsory_roofline_fraction=compulsory / s / HBM))
        print(f"{H}x{W}x{B} ({ps}, {pd}): {med:8.4f} ms ({lo:.4f}-{hi:.4f}), {useful / s / 1e12:6.2f} useful TFLOP/s "
              f"({executed / s / 1e12:.2f} executed), {moved / 1e6:7.1f} MB through the tiles at {moved / s / 1e12:5.2f} TB/s, "
              f"compulsory {compulsory / 1e6:.1f} MB = {compulsory / s / HBM:5.1%} of 6.3 TB/s", flush=True)
    return rows


def time_solver(a):
    """Outer iterations per second of the configs[1] cube with each learning-free low-rank slot (config defaults)."""
    from lrspnp.data import mask_matrix, synthetic_cube, synthetic_dictionary, unfold
    H, W, B, bb = 200, 200, 198, 8
    obs, _, mask = synthetic_cube(H, W, B, seed=0)
    Y, M, D = unfold(obs), mask_matrix(mask, B), synthetic_dictionary(bb * bb, 256, 0)
    out = {}
    for lowrank in ("svt", "tv", "nlm"):
        cfg = LrsPnPConfig(bb=bb, sliding=bb, Nit=80, variant="spec2", lowrank=lowrank, tv=TvProxConfig(),
                           nlm=NlmCubeConfig())
        s = LrsPnP(Y, M, D, cfg, image_shape=(H, W))
        med, lo, hi = median_ms(s.step, a.solver_steps, a.rounds)
        out[lowrank] = dict(ms_per_outer_iteration=med, ms_min=lo, ms_max=hi, outer_iterations_per_s=1e3 / med)
        print(f"configs[1] cube, lowrank={lowrank}: {med:.3f} ms per outer iteration ({lo:.3f}-{hi:.3f}), "
              f"{1e3 / med:.1f}/s", flush=True)
        del s
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cubes", nargs="+", default=["196x196x198", "200x200x198"], help="HxWxB")
    ap.add_argument("--params", nargs="+", default=["7,2", "3,3"], help="patch_size,patch_distance")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--solver-steps", type=int, default=10)
    ap.add_argument("--no-solver", action="store_true")
    ap.add_argument("--out", default=None, help="also write the figures as JSON")
    a = ap.parse_args()
    a.params = [tuple(int(v) for v in p.split(",")) for p in a.params]
    if not torch.cuda.is_available():
        sys.exit("nlmcube_time.py needs the GPU")
    res = {"device": torch.cuda.get_device_name(0), "calls": []}
    for c in a.cubes:
        H, W, B = (int(v) for v in c.split("x"))
        res["calls"] += time_cube(H, W, B, a)
    if not a.no_solver:
        res["solver_200x200x198"] = time_solver(a)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

"""Time of one TV-prox call (ops.tvprox, lrs_tvprox_f32) by device events: median over rounds of several
calls, per term set, iteration count and start (cold / warm), with the time per iteration and the rate of the
compulsory bytes; then the outer iteration of the 200x200x198 cube (BASELINE configs[1]: 8x8
blocks, 80 sparse-coding iterations) with lowrank="svt" and with lowrank="tv", for context.

    python tools/tvprox_time.py [--cubes 196x196x198 200x200x198] [--iters 1 20 50] [--calls 10] [--rounds 7]
                                [--no-solver] [--out profiles/tvprox/tvprox_time.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "lrs-pnp-dip_amd"))
import torch  # noqa: E402
from lrspnp import LrsPnP, LrsPnPConfig, TvProxConfig, ops  # noqa: E402

HBM = 6.3e12   # achievable HBM rate, bytes/s
TERMS = {"sstv": (0.0, 0.0, 1.0), "all": (1.0, 1.0, 1.0)}


def fields(w, H, W, B):
    """The dual fields with array traffic: weight > 0 (every size here is > 1, so no index set is empty)."""
    assert min(H, W, B) > 1
    return 2 * (w[0] > 0) + (w[1] > 0) + 2 * (w[2] > 0)


def call_bytes(n_elem, nf, n_iter, cold, l2=True):
    """Compulsory bytes of one call: every array a pass reads or writes, once.  Z is X (+ L2).  Primal pass:
    Z, the nf fields it gathers, u out.  Dual pass: u, q and p in, p and q out (the first pass of a cold call: Z
    in, p and q out; of a warm call: u and p in, p and q out).  The last pass: Z, p, U out."""
    z = 2 if l2 else 1
    arrays = 0
    for k in range(1, n_iter + 1):
        if k == 1:
            arrays += (z + 2 * nf) if cold else (z + nf + 1) + (1 + nf + 2 * nf)
        else:
            arrays += (z + nf + 1) + (1 + 2 * nf + 2 * nf)
    arrays += z + (nf if n_iter else 0) + 1
    return 4 * n_elem * arrays


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
    ws = ops.tvprox_workspace(H, W, B, "cuda")
    rows = []
    for name, w in TERMS.items():
        nf = fields(w, H, W, B)
        per = {}
        for n in a.iters:
            for start in ("cold", "warm"):
                kw = dict(w_sp=0.05 * w[0], w_bd=0.05 * w[1], w_ss=0.05 * w[2], tau=1.0, U=U)
                ops.tvprox(X, L2, 0.5, H, W, ws, n_iter=max(a.iters), **kw)   # a p for the warm calls to start from
                med, lo, hi = median_ms(lambda: ops.tvprox(X, L2, 0.5, H, W, ws, n_iter=n, warm=start == "warm", **kw),
                                        a.calls, a.rounds)
                nbytes = call_bytes(H * W * B, nf, n, start == "cold")
                per[(n, start)] = med
                rows.append(dict(cube=f"{H}x{W}x{B}", terms=name, fields=nf, n_iter=n, start=start, ms=med, ms_min=lo,
                                 ms_max=hi, ms_per_iter=med / n, compulsory_bytes=nbytes, bytes_per_s=nbytes / (med * 1e-3),
                                 roofline_fraction=nbytes / (med * 1e-3) / HBM))
                print(f"{H}x{W}x{B} {name:4s} n_iter {n:3d} {start}: {med:8.4f} ms ({lo:.4f}-{hi:.4f}), "
                      f"{med / n * 1e3:8.1f} us/iter, {nbytes / 1e6:8.1f} MB compulsory, "
                      f"{nbytes / (med * 1e-3) / 1e12:5.2f} TB/s = {nbytes / (med * 1e-3) / HBM:5.1%} of 6.3 TB/s", flush=True)
        lo_n, hi_n = min(a.iters), max(a.iters)
        if hi_n > lo_n:   # the marginal iteration: the slope between the smallest and the largest count
            us = (per[(hi_n, "cold")] - per[(lo_n, "cold")]) / (hi_n - lo_n) * 1e3
            it_bytes = 4 * H * W * B * (2 + 2 + 5 * nf)
            rows.append(dict(cube=f"{H}x{W}x{B}", terms=name, fields=nf, marginal_us_per_iter=us,
                             iter_bytes=it_bytes, roofline_fraction=it_bytes / (us * 1e-6) / HBM))
            print(f"{H}x{W}x{B} {name:4s} marginal iteration: {us:8.1f} us, {it_bytes / 1e6:.1f} MB compulsory, "
                  f"{it_bytes / (us * 1e-6) / 1e12:5.2f} TB/s = {it_bytes / (us * 1e-6) / HBM:5.1%} of 6.3 TB/s", flush=True)
    return rows


def time_solver(a):
    """Outer iterations per second of the configs[1] cube, SVT against TV prox (TvProxConfig's defaults)."""
    from lrspnp.data import mask_matrix, synthetic_cube, synthetic_dictionary, unfold
    H, W, B, bb = 200, 200, 198, 8
    obs, _, mask = synthetic_cube(H, W, B, seed=0)
    Y, M, D = unfold(obs), mask_matrix(mask, B), synthetic_dictionary(bb * bb, 256, 0)
    out = {}
    for lowrank in ("svt", "tv"):
        cfg = LrsPnPConfig(bb=bb, sliding=bb, Nit=80, variant="spec2", lowrank=lowrank, tv=TvProxConfig())
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
    ap.add_argument("--iters", type=int, nargs="+", default=[1, 20, 50])
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--solver-steps", type=int, default=10)
    ap.add_argument("--no-solver", action="store_true")
    ap.add_argument("--out", default=None, help="also write the figures as JSON")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tvprox_time.py needs the GPU")
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

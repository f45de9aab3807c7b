"""Time of the quality monitor by device events: one ops.cube_quality call on a 196x196x198 cube,
median over rounds of several calls, against its compulsory bytes (X and C once, and the region when given); then
LrsPnP.run(25) with the monitor and the best iterate against 25 bare step() calls, lowrank="svt", on the
200x200x198 cube (BASELINE configs[1]: 8x8 blocks, 80 sparse-coding iterations).

    python tools/quality_time.py [--cube 196x196x198] [--calls 20] [--rounds 7] [--steps 25] [--no-solver]
                                 [--out profiles/quality/quality_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "lrs-pnp-dip_amd"))
import torch  # noqa: E402
from lrspnp import LrsPnP, LrsPnPConfig, ops  # noqa: E402

HBM = 6.3e12   # achievable HBM rate, bytes/s


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


def time_call(H, W, B, a):
    P = H * W
    g = torch.Generator(device="cuda").manual_seed(0)
    X = torch.rand(P, B, device="cuda", generator=g)
    C = torch.rand(P, B, device="cuda", generator=g)
    hole = (torch.rand(P, 1, device="cuda", generator=g) < 0.3).to(torch.uint8).expand(P, B).contiguous()
    ws = ops.cube_quality_workspace(P, B, "cuda")
    q = torch.empty(4, dtype=torch.float64, device="cuda")
    best = torch.full((2,), float("nan"), dtype=torch.float64, device="cuda")
    dst = torch.empty_like(X)
    rows = []
    for name, reg in (("all", None), ("hole", hole)):
        med, lo, hi = median_ms(lambda: ops.cube_quality(X, C, reg, ws=ws, q=q), a.calls, a.rounds)
        nbytes = 4 * P * B * 2 + (P * B if reg is not None else 0)
        floor = nbytes / HBM * 1e3
        rows.append(dict(call="cube_quality", cube=f"{H}x{W}x{B}", region=name, ms=med, ms_min=lo, ms_max=hi,
                         compulsory_bytes=nbytes, floor_ms=floor, fraction_of_floor_rate=floor / med))
        print(f"cube_quality {H}x{W}x{B} region={name}: {med * 1e3:8.2f} us ({lo * 1e3:.2f}-{hi * 1e3:.2f}); "
              f"compulsory {nbytes / 1e6:.1f} MB = {floor * 1e3:.2f} us at 6.3 TB/s: {floor / med:5.1%} of that rate",
              flush=True)
    # keep_best when the score is not better (two launches that write nothing) and when it is (the copy)
    q.fill_(1.0)
    best.copy_(torch.tensor([2.0, 0.0], dtype=torch.float64))
    med, lo, hi = median_ms(lambda: ops.keep_best(q[:1], 1, 0, X, dst, best), a.calls, a.rounds)
    rows.append(dict(call="keep_best", better=False, ms=med, ms_min=lo, ms_max=hi))
    print(f"keep_best, not better: {med * 1e3:8.2f} us ({lo * 1e3:.2f}-{hi * 1e3:.2f})", flush=True)

    def kept():
        best.fill_(float("nan"))
        ops.keep_best(q[:1], 1, 0, X, dst, best)
    med, lo, hi = median_ms(kept, a.calls, a.rounds)
    rows.append(dict(call="keep_best", better=True, ms=med, ms_min=lo, ms_max=hi, bytes=8 * P * B))
    print(f"keep_best, better (with the fill of best): {med * 1e3:8.2f} us ({lo * 1e3:.2f}-{hi * 1e3:.2f}); "
          f"{8 * P * B / 1e6:.1f} MB read and written", flush=True)
    return rows


def time_solver(a):
    """run(steps) with MPSNR on the hole and the best iterate kept, against the same number of bare step() calls:
    device time between events, and the host's wall time to enqueue and finish."""
    from lrspnp.data import mask_matrix, synthetic_cube, synthetic_dictionary, unfold
    H, W, B, bb = 200, 200, 198, 8
    obs, clean, mask = synthetic_cube(H, W, B, seed=0)
    Y, M, D = unfold(obs), mask_matrix(mask, B), synthetic_dictionary(bb * bb, 256, 0)
    clean_u = torch.from_numpy(unfold(clean)).cuda()
    cfg = LrsPnPConfig(bb=bb, sliding=bb, Nit=80, variant="spec2", lowrank="svt")
    s = LrsPnP(Y, M, D, cfg)

    def bare():
        for _ in range(a.steps):
            s.step()

    def monitored():
        s.run(a.steps, clean_u, region="hole", keep_best="mpsnr")

    out = {}
    for name, fn in (("step", bare), ("run", monitored), ("step_again", bare), ("run_again", monitored)):
        fn()
        torch.cuda.synchronize()
        res = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            res.append((e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3))
        dev, wall = statistics.median(r[0] for r in res), statistics.median(r[1] for r in res)
        out[name] = dict(steps=a.steps, device_ms=dev, wall_ms=wall, device_ms_per_iteration=dev / a.steps)
        print(f"configs[1] cube, svt, {a.steps} x {name}: {dev:.2f} ms between events ({dev / a.steps:.3f} per "
              f"iteration), {wall:.2f} ms wall", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cube", default="196x196x198", help="HxWxB")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--no-solver", action="store_true")
    ap.add_argument("--out", default=None, help="also write the figures as JSON")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("quality_time.py needs the GPU")
    H, W, B = (int(v) for v in a.cube.split("x"))
    res = {"device": torch.cuda.get_device_name(0), "calls": time_call(H, W, B, a)}
    if not a.no_solver:
        res["solver_200x200x198"] = time_solver(a)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

"""Accelerated (FISTA) against plain sparse coding on the benchmark shapes (a timing tool, not a test).

    python tools/micro/ista_accel.py [--rounds 5] [--calls 10] [--only cfg2]

Shapes: configs[2]'s sparse coding (196x196x198 cube, 6,408 blocks of 36^2, K = 256, the tiled
mask's patterns, Nit 100) on the per-pattern kernel the solver picks and on the row-split kernel, and
configs[1]'s (200x200x198, 125,000 blocks of 8^2, K = 256, Nit 80), where the plain call runs the
dictionary-resident kernel and the accelerated call the row-split kernel; configs[3]'s (512x512x224,
50,974 blocks of 36^2) on the row-split kernel, time only: its 3,186 tiles select three waves per
workgroup, the accelerated K = 256 form that is bounded for one wave per SIMD instead of two.  Per shape,
one JSON line each:

1. "time": lrs_ista_opts.accel = FISTA against NONE at equal Nit, same build, the two alternating
   inside every round (HIP events around `calls` back-to-back launches; median and range per call
   over the rounds).  At configs[1] this is the row-split kernel against k_ista_ln2.
2. "nit": with the soft threshold, the mean lasso objective ||m .* (y - D x)||^2 + lambda ||x||_1
   of ISTA at Nit = 100 and the smallest Nit at which FISTA's is at or below it (every Nit from 1 is
   run; the sweep is not timed).
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [REPO, os.path.join(REPO, "lrs-pnp-dip_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from lrspnp import LrsPnP, LrsPnPConfig, ops  # noqa: E402
from lrspnp.data import load_fixture, mask_matrix, synthetic_cube, synthetic_dictionary, unfold  # noqa: E402

LAMBDA = 0.1


def solver(H, W, B, bb, nit, variant, patterns):
    base = load_fixture("data_img5.npz")["lrs_mask"]
    obs, _, mask = synthetic_cube(H, W, B, seed=0, base_mask=base)
    s = LrsPnP(unfold(obs), mask_matrix(mask, B), synthetic_dictionary(bb * bb, 256, 0),
               LrsPnPConfig(bb=bb, sliding=bb, Nit=nit, variant=variant, ista_patterns=patterns))
    ops.im2col(s.X, s.L1, s.mu1_32, bb, s.rows_d, s.cols_d, s.n_pad, Yb=s.Yb)
    return s


def coder(s):
    """call(Nit, accel) -> (phi, coefs) on the path the solver picked, workspaces made once."""
    if s.pat_plan is not None:
        return "k_ista_pat", lambda nit, accel: ops.ista_pat(
            s.Yb, s.obs_pat, s.pat_plan, s.pat_ntiles, s.K, s.n, s.alpha, s.thr, nit, s.ista_ws, s.prox, phi=s.phi,
            want_coefs=True, accel=accel)
    ws = {a: ops.ista_workspace(s.n, s.K, s.prox, s.Yb.device, accel=a) for a in ("off", "fista")}
    name = "k_ista_rs" if ws["off"] is not None else "resident (off) / k_ista_rs (fista)"
    return name, lambda nit, accel: ops.ista(s.Yb, s.obs, s.D, s.n, s.alpha, s.thr, nit, s.prox, phi=s.phi,
                                             want_coefs=True, ws=ws[accel], accel=accel)


def time_pair(call, nit, rounds, calls):
    st = torch.cuda.current_stream()
    for a in ("off", "fista"):
        call(nit, a)
    torch.cuda.synchronize()
    ms = {"off": [], "fista": []}
    for r in range(rounds):
        for a in (("off", "fista") if r % 2 == 0 else ("fista", "off")):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(calls):
                call(nit, a)
            e1.record(st)
            torch.cuda.synchronize()
            ms[a].append(e0.elapsed_time(e1) / calls)
    return {a: {"median_ms": float(np.median(v)), "min_ms": min(v), "max_ms": max(v)} for a, v in ms.items()}


def mean_objective(s, phi, coefs):
    r = torch.where(s.obs != 0, s.Yb.double() - phi.double(), torch.zeros((), dtype=torch.float64, device=phi.device))
    return float(((r * r).sum(1) + LAMBDA * coefs.double().abs().sum(1)).mean())


def nit_sweep(s, call, nit_ref=100):
    ref = mean_objective(s, *call(nit_ref, "off"))
    at = {}
    for nit in range(1, nit_ref + 1):
        at[nit] = mean_objective(s, *call(nit, "fista"))
        if at[nit] <= ref:
            return {"ista_objective_at_100": ref, "fista_nit": nit, "fista_objective": at[nit],
                    "fista_objective_at_100": mean_objective(s, *call(nit_ref, "fista"))}
    return {"ista_objective_at_100": ref, "fista_nit": None, "fista_objective_at_100": at[nit_ref]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    jobs = [("cfg2_196x196x198_bb36_pattern", 196, 196, 198, 36, 100, "fro4", "auto"),
            ("cfg2_196x196x198_bb36_rowsplit", 196, 196, 198, 36, 100, "fro4", "off"),
            ("cfg1_200x200x198_bb8", 200, 200, 198, 8, 80, "spec2", "auto"),
            ("cfg3_512x512x224_bb36_rowsplit_timeonly", 512, 512, 224, 36, 100, "fro4", "off")]
    for name, H, W, B, bb, nit, variant, patterns in jobs:
        if a.only and a.only not in name:
            continue
        s = solver(H, W, B, bb, nit, variant, patterns)
        kern, call = coder(s)
        print(json.dumps({"workload": name, "what": "time", "kernel": kern, "blocks": s.nb, "Nit": nit,
                          "variant": variant, **time_pair(call, nit, a.rounds, a.calls)}), flush=True)
        if name.endswith("timeonly"):
            continue
        s = solver(H, W, B, bb, nit, "soft", patterns)
        kern, call = coder(s)
        print(json.dumps({"workload": name, "what": "nit", "kernel": kern, "variant": "soft", **nit_sweep(s, call)}),
              flush=True)


if __name__ == "__main__":
    main()

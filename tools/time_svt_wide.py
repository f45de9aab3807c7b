"""Time the phases of the SVT prox on wide cubes (256 < B <= 512), alone on the GPU, with HIP events:
the Gram (lrs_svt_gram_f32), the eigen stage cold and warm, and the apply U = Z (I - E), beside the
same phases of the existing path at B = 256.

    python tools/time_svt_wide.py [--P 40000] [--reps 3] [--out FILE.json]

Per shape, median of --reps:
  gram        lrs_svt_gram_f32, cold (Gram + fixed-order reduce)
  gram_warm   the same with LRS_SVT_WARM (wide cubes, and 'jacobi' at 256: + the products V^T (G V))
  eig_cold    lrs_svt_finish_f32 cold minus the apply alone (one stream: its kernels run in order)
  eig_warm    the same after a cold solve, on the matrix perturbed by 1e-3 N(0, 1)
  apply       the apply kernel alone (lrs_diag_svt_apply)
  sweeps      Jacobi sweeps cold / warm (0 on the tridiagonal path)
At B = 256 both solvers of the existing path are timed: 'tri' (the default there; no warm start) and
'jacobi' (the chain the wide cubes run).  Every wide shape is timed with its three eigen stages: the
default Jacobi chain ('tri' row, path 3), the tridiagonal chain of LRS_SVT_WIDE_TRI ('wide_tri' row,
path 4; its "warm" column is the same cold chain on the perturbed matrix: it takes no warm start) and
that chain with the many-workgroup Householder reduction of LRS_SVT_WIDE_MW ('wide_mw' row, path 4,
state word 7 set).
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "lrs-pnp-dip_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from lrspnp import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--P", type=int, default=40000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=None)
a = ap.parse_args()

C2 = float(np.float32(1 / 0.9))
TAU = C2
st = torch.cuda.current_stream()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    fn()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def shape(P, B, method, wide_tri=False, wide_mw=False):
    rng = np.random.default_rng(P + B)
    Z = rng.random((P, 8)) @ rng.random((8, B)) * 0.3 + 0.02 * rng.standard_normal((P, B))
    X = torch.from_numpy(Z.astype(np.float32)).cuda()
    X2 = torch.from_numpy((Z + 1e-3 * rng.standard_normal((P, B))).astype(np.float32)).cuda()
    L2 = torch.from_numpy((0.01 * rng.standard_normal((P, B))).astype(np.float32)).cuda()
    U = torch.empty_like(X)
    ws = ops.svt_workspace(P, B, "cuda")
    kw = {"method": method, "wide_tri": wide_tri, "wide_mw": wide_mw}
    ops.svt(X, L2, C2, TAU, ws, U=U, **kw)   # first launches (module load, LDS opt-in)
    torch.cuda.synchronize()
    t = {k: [] for k in ("gram", "gram_warm", "fin_cold", "fin_warm", "apply")}
    sweeps = [0, 0]
    warmable = method == "jacobi" or B > 256
    for _ in range(a.reps):
        t["gram"].append(timed(lambda: ops.svt_gram(X, L2, C2, ws, **kw)))
        t["fin_cold"].append(timed(lambda: ops.svt_finish(X, L2, C2, TAU, ws, U, **kw)))
        state = ops.svt_state(ws, P, B)
        path, sweeps[0] = state[4], state[3] if state[4] not in (1, 4) else 0
        if warmable:
            t["gram_warm"].append(timed(lambda: ops.svt_gram(X2, L2, C2, ws, warm=True, **kw)))
            t["fin_warm"].append(timed(lambda: ops.svt_finish(X2, L2, C2, TAU, ws, U, warm=True, **kw)))
            state = ops.svt_state(ws, P, B)
            sweeps[1] = state[3] if state[4] != 4 else 0
        t["apply"].append(timed(lambda: ops.svt_apply_only(X2, L2, C2, ws, U)))
    m = {k: float(np.median(v)) if v else None for k, v in t.items()}
    assert state[7] == int(wide_mw), state[:8]
    return {"P": P, "B": B, "method": "wide_mw" if wide_mw else "wide_tri" if wide_tri else method, "path": path,
            "ws_MB": ws.numel() / 1e6,
            "gram_ms": m["gram"], "gram_warm_ms": m["gram_warm"],
            "eig_cold_ms": m["fin_cold"] - m["apply"],
            "eig_warm_ms": m["fin_warm"] - m["apply"] if warmable else None,
            "apply_ms": m["apply"], "sweeps_cold": sweeps[0], "sweeps_warm": sweeps[1] if warmable else None}


rows = [shape(a.P, 256, "tri"), shape(a.P, 256, "jacobi")]
for B in (320, 448, 512):
    rows.append(shape(a.P, B, "tri"))
    rows.append(shape(a.P, B, "tri", wide_tri=True))
    rows.append(shape(a.P, B, "tri", wide_tri=True, wide_mw=True))
f = lambda v: "     -" if v is None else f"{v:6.0f}" if isinstance(v, int) else f"{v:9.3f}"
print(f"{'P':>6} {'B':>4} {'solver':>8} {'path':>4} {'ws MB':>9} {'gram':>9} {'gram warm':>9} {'eig cold':>9} "
      f"{'eig warm':>9} {'apply':>9} {'sweeps c/w':>10}   (ms, median of {a.reps})")
for r in rows:
    print(f"{r['P']:6d} {r['B']:4d} {r['method']:>8} {r['path']:4d} {f(r['ws_MB'])} {f(r['gram_ms'])} "
          f"{f(r['gram_warm_ms'])} {f(r['eig_cold_ms'])} {f(r['eig_warm_ms'])} {f(r['apply_ms'])} "
          f"{r['sweeps_cold']:>5}/{'-' if r['sweeps_warm'] is None else r['sweeps_warm']}")
    print(json.dumps(r))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rows, fh, indent=1)

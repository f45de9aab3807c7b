#!/usr/bin/env python3
"""Measurements of the dictionary learning recorded in DESIGN.md §8 (run on the MI355X):

  round : HIP-event time of one round at configs[2]'s cube (196x196x198, 36x36 blocks, K = 256,
          train_sliding = 12), split into the step size (lrs_ista_alpha_f32), the sparse coding and
          the dictionary step (lrs_dict_stats_f32 + lrs_dict_update_f32, n_inner = 10);
  mpsnr : configs[1] (200x200x198 cube, 8x8 blocks, K = 256, Nit 80, SVT) after --outer iterations
          with the dictionary learned from the observation against the synthetic stand-in.

Prints one JSON line per measurement.  Inputs are bench.py's seeded synthetic cube and tiled mask."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lrs-pnp-dip_amd"))


def problem(H, W, B):
    from lrspnp.data import load_fixture, mask_matrix, synthetic_cube, unfold
    base = load_fixture("data_img5.npz")["lrs_mask"]
    obs, clean, mask = synthetic_cube(H, W, B, seed=0, base_mask=base)
    return unfold(obs), mask_matrix(mask, B), clean


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for r in range(reps):
        fn()
        ev[r + 1].record()
    torch.cuda.synchronize()
    return sorted(ev[r].elapsed_time(ev[r + 1]) for r in range(reps))[reps // 2]


def measure_round(a):
    import torch
    from lrspnp import DictLearnConfig, ops
    from lrspnp.dictlearn import initial_dictionary, training_blocks
    Y, M, _ = problem(196, 196, 198)
    cfg = DictLearnConfig(K=256, bb=36, train_sliding=12, Nit=100, n_inner=10)
    rng = np.random.default_rng(0)
    dev = torch.device("cuda")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    Yb, obs, n_pad = training_blocks(t(Y), t(M), cfg, rng)
    nb, n, K = Yb.shape[0], 1296, 256
    D = t(initial_dictionary(Yb, obs, n, K, rng))
    packed = np.packbits(obs.cpu().numpy(), axis=1)
    uniq, inv = np.unique(packed, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    npat = uniq.shape[0]
    obs_pat = t(np.unpackbits(uniq, axis=1)[:, :n_pad].astype(np.uint8))
    inv_d = t(inv.astype(np.int64))
    per_pattern = ops.ista_pat_preferred(n, K, nb, npat, cfg.Nit)
    coefs = torch.zeros((nb, K), dtype=torch.float32, device=dev)
    phi = torch.empty((nb, n_pad), dtype=torch.float32, device=dev)
    ws = ops.dict_workspace(n, n_pad, K, nb, dev)
    st = {}

    def alpha():
        ap, tp = ops.ista_alpha(D, obs_pat, n, ops.ALPHA_SOFT, cfg.lambda_ista)
        st["alpha"], st["thr"] = ap.index_select(0, inv_d), tp.index_select(0, inv_d)

    if per_pattern:
        plan, ntiles = ops.ista_pat_plan(inv, npat)
        plan_d = t(plan)
        iws = ops.ista_pat_workspace(n, K, npat, dev)

        def code():
            ops.ista_pat_prepare(D, obs_pat, n, ws=iws)
            ops.ista_pat(Yb, obs_pat, plan_d, ntiles, K, n, st["alpha"], st["thr"], cfg.Nit, iws, ops.PROX_SOFT,
                         phi=phi, coefs=coefs, want_coefs=True)
    else:
        iws = ops.ista_workspace(n, K, ops.PROX_SOFT, dev)

        def code():
            ops.ista(Yb, obs, D, n, st["alpha"], st["thr"], cfg.Nit, ops.PROX_SOFT, phi=phi, coefs=coefs,
                     want_coefs=True, ws=iws)

    Dw = D.clone()

    def step():
        Dw.copy_(D)
        _, c = ops.dict_stats(coefs, ws=ws)
        ops.dict_update(Yb, obs, coefs, Dw, n, c, cfg.n_inner, ws=ws)

    ms = {"alpha": timed(alpha, a.reps), "sparse_coding": timed(code, a.reps), "dictionary_step": timed(step, a.reps)}
    ms["round"] = sum(ms.values())
    print(json.dumps({"measure": "round", "cube": "196x196x198", "bb": 36, "K": K, "train_sliding": 12, "blocks": nb,
                      "patterns": npat, "sparse_coding_kernel": "per-pattern" if per_pattern else "row-split",
                      "Nit": cfg.Nit, "n_inner": cfg.n_inner, "median_ms": ms, "reps": a.reps}))


def measure_mpsnr(a):
    import torch
    from lrspnp import DictLearnConfig, LrsPnP, LrsPnPConfig
    from lrspnp.data import synthetic_dictionary
    from lrspnp.metrics import mpsnr
    Y, M, clean = problem(200, 200, 198)
    clean_d = torch.from_numpy(clean).cuda()
    out = {"measure": "mpsnr", "cube": "200x200x198", "bb": 8, "K": 256, "Nit": 80, "outer": a.outer,
           "input": mpsnr(torch.from_numpy(Y).cuda(), clean_d)}
    dcfg = DictLearnConfig(K=256, rounds=a.rounds)
    for name, D in (("synthetic", synthetic_dictionary(64, 256, 0)), ("learned", "learn")):
        t0 = time.time()
        s = LrsPnP(Y, M, D, LrsPnPConfig(bb=8, sliding=8, Nit=80, variant="spec2", dict_cfg=dcfg))
        torch.cuda.synchronize()
        setup = time.time() - t0
        for _ in range(a.outer):
            s.step()
        torch.cuda.synchronize()
        out[name] = {"mpsnr": mpsnr(s.X, clean_d), "setup_s": round(setup, 2)}
        if s.dict_history is not None:
            out[name]["objective"] = [float(s.dict_history[0, 0]), float(s.dict_history[-1, -1])]
            out[name]["rounds"] = a.rounds
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("what", choices=["round", "mpsnr"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--outer", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=20)
    measure_round(ap.parse_args()) if ap.parse_args().what == "round" else measure_mpsnr(ap.parse_args())

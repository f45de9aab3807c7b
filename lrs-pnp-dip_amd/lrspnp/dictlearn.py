"""Masked dictionary learning on one MI355X (host orchestration only).

The reference loads its sparsifying dictionary from ``trained_dictionary.mat``
(main_LRS_PnP.py:159-160), a file that was never published together with its training code.
``learn_dictionary`` produces one from the noisy, incomplete observation itself, by alternating
minimisation of

    F(D, A) = sum_j 1/2 ||m_j .* (y_j - D a_j)||^2 + lambda ||a_j||_1,   ||d_k||_2 <= 1

over raw (no mean removed) training blocks y_j of the observed unfolded cube:

* sparse coding with the solver's own kernels (``ops.ista_alpha`` with ALPHA_SOFT for the current D,
  then ``ops.ista`` / ``ops.ista_pat`` with PROX_SOFT);
* the dictionary step of ``ops.dict_stats`` / ``ops.dict_update`` (majorisation-minimisation with
  the mask inside the residual, step 1 / c with c >= lambda_max(A^T A)).

The host draws the training blocks and the initial atoms once, groups the blocks by observation
pattern once, enqueues the rounds without synchronising, and reads the objective history once at
the end.

Warm start.  From the second round on the sparse coding continues from the previous round's
coefficients where the kernel can (``lrs_ista_opts.warm_start``): the row-split kernel of
``lrs_ista_f32`` (n_pad > 64 or K != 256) and the per-pattern kernel of ``lrs_ista_pat_f32``.  The
dictionary-resident kernels (n_pad <= 64 with K = 256) start every round from zero.

``DictLearnConfig.accel = "fista"`` runs every round's sparse coding with Nesterov momentum
(``lrs_ista_opts.accel``).  The warm start between rounds then carries the coefficients only: the
momentum restarts in every call, which is the right thing after D has changed.  Accelerated calls
run the row-split kernel at the resident sizes too, so they warm-start at every K <= 512.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import ops
from ._lib import LrsError


@dataclass
class DictLearnConfig:
    K: int = 256                     # atoms
    bb: int = 36                     # block size (n = bb * bb rows of D)
    train_sliding: int | None = None  # stride of the training grid (None: bb // 3)
    max_blocks: int = 65536          # seeded subsample of the grid above this many blocks
    lambda_ista: float = 0.1         # ISTA lambda, as LrsPnPConfig.lambda_ista
    Nit: int = 100                   # ISTA iterations per round
    rounds: int = 20                 # sparse coding + dictionary step
    n_inner: int = 10                # majorisation-minimisation iterations per dictionary step
    normalise: bool = True           # unit-norm columns at the end (columnNormalise.m)
    accel: str = "off"               # per-round sparse coding: "off" (ISTA) or "fista" (lrs_ista_opts.accel)
    seed: int = 0


def warm_start_supported(n_pad: int, K: int, per_pattern: bool, accel: str = "off") -> bool:
    """Whether the sparse-coding kernel these sizes select continues from given coefficients
    (accelerated calls never run the resident kernels)."""
    return per_pattern or n_pad > 64 or K != 256 or accel != "off"


def training_blocks(Y, M, cfg: DictLearnConfig, rng):
    """(Yb, obs, n_pad): the training blocks of the observed cube Y (P, B) and their 0/1 observation
    masks from M, on the training grid of stride cfg.train_sliding, subsampled to cfg.max_blocks."""
    P, B = Y.shape
    n = cfg.bb * cfg.bb
    n_pad = -(-n // 16) * 16
    stride = int(cfg.train_sliding) if cfg.train_sliding else max(1, cfg.bb // 3)
    rows, cols = ops.block_grid(P, B, cfg.bb, stride)
    if rows.size > cfg.max_blocks:
        keep = np.sort(rng.choice(rows.size, int(cfg.max_blocks), replace=False))
        rows, cols = rows[keep], cols[keep]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(Y.device)
    rows_d, cols_d = t(rows), t(cols)
    Yb = ops.im2col(Y, None, 1.0, cfg.bb, rows_d, cols_d, n_pad)
    _, obs = ops.im2col(M, None, 1.0, cfg.bb, rows_d, cols_d, n_pad, want_obs=True)
    return Yb, obs, n_pad


def initial_dictionary(Yb, obs, n: int, K: int, rng) -> np.ndarray:
    """K distinct seeded training blocks, missing entries filled with the block's observed mean, unit
    norm (host, once).  Blocks with nothing observed or a zero norm are passed over."""
    nb = Yb.shape[0]
    order = rng.permutation(nb)
    atoms = []
    for lo in range(0, nb, 4 * K):
        idx = torch.from_numpy(np.sort(order[lo: lo + 4 * K])).to(Yb.device)
        yb = Yb.index_select(0, idx).cpu().numpy()[:, :n].astype(np.float64)
        ob = obs.index_select(0, idx).cpu().numpy()[:, :n] != 0
        for y, o in zip(yb, ob):
            if not o.any():
                continue
            a = np.where(o, y, y[o].mean())
            nrm = np.linalg.norm(a)
            if nrm > 0:
                atoms.append(a / nrm)
            if len(atoms) == K:
                return np.ascontiguousarray(np.stack(atoms, axis=1), dtype=np.float32)
    raise LrsError(f"initial dictionary: {len(atoms)} usable training blocks for K = {K} atoms "
                   "(lower train_sliding, or pass D0)")


def learn_blocks(Yb, obs, n: int, D0, cfg: DictLearnConfig):
    """The rounds on given training blocks Yb (nb, n_pad) f32, obs (nb, n_pad) u8 and initial
    dictionary D0 (n, K), all on the device.  Returns (D, history) as device tensors: D (n, K) float32
    and the objective 1/2 ||obs .* (Yb - A D^T)||^2 as (rounds, n_inner + 1) float64.  No host
    synchronisation after the one-off pattern grouping."""
    dev = Yb.device
    nb, n_pad = Yb.shape
    D = D0.detach().clone().contiguous()
    K = D.shape[1]
    if D.shape[0] != n:
        raise LrsError(f"dictionary has {D.shape[0]} rows, expected {n}")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    # ---- blocks grouped by observation pattern (host, once): alpha and the threshold are per pattern
    packed = np.packbits(obs.cpu().numpy(), axis=1)
    uniq, inv = np.unique(packed, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    npat = uniq.shape[0]
    obs_pat = t(np.unpackbits(uniq, axis=1)[:, :n_pad].astype(np.uint8))
    inv_d = t(inv.astype(np.int64))
    per_pattern = K <= 512 and ops.ista_pat_preferred(n, K, nb, npat, cfg.Nit)   # the solver's own rule
    if cfg.accel not in ("off", "fista"):
        raise LrsError(f"unknown accel {cfg.accel!r} (off | fista)")
    warm_ok = warm_start_supported(n_pad, K, per_pattern, cfg.accel)
    if per_pattern:
        plan, ntiles = ops.ista_pat_plan(inv, npat)
        plan_d = t(plan)
        ista_ws = ops.ista_pat_workspace(n, K, npat, dev)
    else:
        ista_ws = ops.ista_workspace(n, K, ops.PROX_SOFT, dev, accel=cfg.accel)
    coefs = torch.zeros((nb, K), dtype=torch.float32, device=dev)
    phi = torch.empty((nb, n_pad), dtype=torch.float32, device=dev)
    H = torch.empty((K, K), dtype=torch.float32, device=dev)
    c = torch.empty(1, dtype=torch.float64, device=dev)
    ws = ops.dict_workspace(n, n_pad, K, nb, dev)
    rounds, n_inner = int(cfg.rounds), int(cfg.n_inner)
    history = torch.zeros((rounds, n_inner + 1), dtype=torch.float64, device=dev)
    for r in range(rounds):
        alpha_pat, thr_pat = ops.ista_alpha(D, obs_pat, n, ops.ALPHA_SOFT, cfg.lambda_ista)
        alpha = alpha_pat.index_select(0, inv_d)
        thr = thr_pat.index_select(0, inv_d)
        warm = warm_ok and r > 0
        if per_pattern:
            ops.ista_pat_prepare(D, obs_pat, n, ws=ista_ws)
            ops.ista_pat(Yb, obs_pat, plan_d, ntiles, K, n, alpha, thr, cfg.Nit, ista_ws, ops.PROX_SOFT, phi=phi,
                         coefs=coefs, want_coefs=True, warm_start=warm, accel=cfg.accel)
        else:
            ops.ista(Yb, obs, D, n, alpha, thr, cfg.Nit, ops.PROX_SOFT, phi=phi, coefs=coefs, want_coefs=True,
                     ws=ista_ws, warm_start=warm, accel=cfg.accel)
        ops.dict_stats(coefs, H=H, c=c, ws=ws)
        ops.dict_update(Yb, obs, coefs, D, n, c, n_inner, obj=history[r], ws=ws)
    if cfg.normalise:
        ops.dict_normalise(D)
    return D, history


def learn_dictionary(Y, M, cfg: DictLearnConfig | None = None, D0=None, device="cuda"):
    """Learn an n x K dictionary (n = bb * bb) from the observed unfolded cube Y (P, B; zeros at
    missing entries) and its 0/1 mask M (P, B).  D0: an initial dictionary (n, K), else K seeded
    training blocks.  Returns (D, history): D a float32 device tensor, history a (rounds,
    n_inner + 1) float64 numpy array of the masked objective, read from the device once."""
    cfg = cfg or DictLearnConfig()
    dev = torch.device(device)
    f = lambda a: torch.as_tensor(np.asarray(a, np.float32) if not isinstance(a, torch.Tensor) else a,
                                  dtype=torch.float32).to(dev).contiguous()
    Y, M = f(Y), f(M)
    if Y.shape != M.shape or Y.dim() != 2:
        raise LrsError(f"Y {tuple(Y.shape)} and M {tuple(M.shape)} must be the same (P, B) matrices")
    n = cfg.bb * cfg.bb
    rng = np.random.default_rng(cfg.seed)
    Yb, obs, _ = training_blocks(Y, M, cfg, rng)
    if D0 is None:
        if Yb.shape[0] < cfg.K:
            raise LrsError(f"{Yb.shape[0]} training blocks for K = {cfg.K} atoms (lower train_sliding, or pass D0)")
        D0 = initial_dictionary(Yb, obs, n, int(cfg.K), rng)
    D0 = f(D0)
    if tuple(D0.shape) != (n, int(cfg.K)):
        raise LrsError(f"D0 is {tuple(D0.shape)}, expected ({n}, {cfg.K})")
    D, history = learn_blocks(Yb, obs, n, D0, cfg)
    return D, history.cpu().numpy()

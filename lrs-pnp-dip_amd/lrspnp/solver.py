"""Batched LRS-PnP ADMM outer loop on one MI355X (host orchestration only).

Mirrors the module-level loop of main_LRS_PnP.py:244-366 (SVT low-rank prox) with the DIP
variants' ISTA rule selectable (…1-LiP.py:185-198).  One `step()` = one outer ADMM iteration:

    main stream : im2col(X + L1/mu1) -> fused masked ISTA + PnP prox (all blocks) -> Phi
    lowrank str.: SVT(X + L2/mu2, 1/mu2) -> U            (runs concurrently with the ISTA)
    main stream : col2im + closed-form X + dual updates + ||delta||^2   (waits for both)

No per-block Python, no host synchronisation inside `step()`.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import ops
from ._lib import LrsError
from .dip import stream_wait


@dataclass
class TvProxConfig:
    """lowrank='tv': the weights of the cube's spatial, band and spatial-spectral TV in U = prox_{T / mu2}
    (ops.tvprox), the fixed number of dual iterations per outer iteration, and whether an outer iteration
    starts from the previous one's dual variable.  A starting point: no quality claim rests on these values."""
    w_sp: float = 0.0
    w_bd: float = 0.0
    w_ss: float = 1.0
    n_iter: int = 20
    warm: bool = True


@dataclass
class NlmCubeConfig:
    """lowrank='nlm': the patch size, search radius, filter strength h and noise level sigma of the spectral
    non-local means U = NLM(X + L2/mu2) (ops.nlmcube).  The defaults are the reference's own call
    (admm_utils.py:95-100, which it never makes): no quality claim rests on them.  The slot's tau = 1/mu2 is
    NOT used: sigma is this config's own and is not coupled to mu2."""
    patch_size: int = 7
    patch_distance: int = 2
    h: float = 0.05
    sigma: float = 0.0

    def check(self):
        """LrsError for a value lrs_nlmcube_f32 would refuse (host-only)."""
        if int(self.patch_size) != self.patch_size or self.patch_size not in (1, 3, 5, 7):
            raise LrsError(f"NlmCubeConfig.patch_size must be 1, 3, 5 or 7, got {self.patch_size!r}")
        if int(self.patch_distance) != self.patch_distance or not 0 <= self.patch_distance <= 5:
            raise LrsError(f"NlmCubeConfig.patch_distance must be 0..5, got {self.patch_distance!r}")
        if not (self.h > 0 and np.isfinite(self.h)):
            raise LrsError(f"NlmCubeConfig.h must be positive and finite, got {self.h!r}")
        if not self.sigma >= 0:
            raise LrsError(f"NlmCubeConfig.sigma must be >= 0, got {self.sigma!r}")


@dataclass
class LrsPnPConfig:
    """The knob table of SURVEY.md §5 (main_LRS_PnP.py:218-238 defaults)."""
    gamma: float = 0.5            # data fidelity                      main_LRS_PnP.py:218
    mu1: float = 0.15             # sparsity penalty                   :221
    mu2: float = 0.15 * 6         # low-rank penalty                   :222
    lambda_ista: float = 0.1      # ISTA lambda                         :225
    Nit: int = 80                 # inner ISTA iterations               :226
    bb: int = 36                  # block size                          :237
    sliding: int = 36             # slidingDis                          :238
    variant: str = "spec2"        # 'spec2' (main), 'fro4' (DIP mains), 'soft' (ista.m), 'matlab' (pnp_ista.m)
    svt_method: str = "tri"       # SVT eigensolver: 'tri' (tridiagonal, certified) or 'jacobi'
    svt_warm: bool = True         # warm-start the Jacobi eigensolver from the previous iteration
    svt_gram_first: bool = False  # hold the sparse coding until the SVT Gram is done (always for Jacobi)
    # The tridiagonal eigensolver's eigenvalue / inverse-iteration / back-transformation phases over
    # many workgroups (LRS_SVT_MULTI_WG, bit-identical): "auto" on a row-slab shard, where the
    # replicated solve is on the critical path; the one-workgroup chain beside a whole-cube sparse
    # coding (a multi-launch chain there waits for free CUs between its launches).
    svt_multi_wg: str = "auto"
    # eigen stage of wide cubes (256 < B <= 512; ignored below): 'jacobi', the warm-started
    # one-workgroup Jacobi chain, 'tri', the tridiagonal chain over many workgroups (LRS_SVT_WIDE_TRI), or
    # 'tri-mw', that chain with its Householder reduction over many workgroups too (+ LRS_SVT_WIDE_MW)
    svt_wide_solver: str = "jacobi"
    # 'svt' (main_LRS_PnP.py:315), 'dip' (…1-LiP.py:399-411), 'tv' (TV prox on the cube) or 'nlm' (spectral NLM on it)
    lowrank: str = "svt"
    dip: object = None            # lrspnp.dip.DipConfig for lowrank='dip' (None: reference defaults)
    tv: object = None             # TvProxConfig for lowrank='tv' (None: its defaults); the dip fields are ignored there
    nlm: object = None            # NlmCubeConfig for lowrank='nlm' (None: its defaults)
    dip_seed: int = 0             # DIP init seed of outer iteration t is dip_seed + t
    # Workgroups of the sparse-coding kernel beside the DIP training (lowrank='dip';
    # lrs_ista_opts.max_workgroups, 0 = one per 16-block tile).  Measured at configs[2]
    # (bench.py --ista-max-wg): 0 -> 7.25 outer it/s, 128 -> 7.18, 64 -> 6.97, 32 -> 6.68: a longer,
    # narrower sparse coding taxes the DIP more than a short full-chip one, so unbounded.  Re-measured
    # on the per-pattern kernel (405 tiles, 3 interleaved rounds, profiles/r04/ista_max_wg/):
    # 0 -> 7.85 / 7.84 / 7.84, 256 -> 7.84 / 7.84 / 7.82, 128 -> 7.80 / 7.81 / 7.80.
    ista_max_wg_dip: int = 0
    # Launches the sparse coding's Nit iterations are split over beside the DIP training
    # (lowrank='dip'; lrs_ista_opts.warm_start: the iterates are exactly those of one launch).  A
    # workgroup of one launch holds its CU for the whole Nit; slices free CUs for the DIP's kernels
    # every Nit / slices iterations.  Measured at configs[2] (bench.py --ista-slices, 2 rounds):
    # 1 -> 7.50 outer it/s, 4 -> 7.49, 10 -> 7.39-7.42, 25 -> 7.27 (each slice re-forms D^T(m.*y) and
    # Phi, and runs longer beside the DIP than its share of one launch), so one launch.
    ista_slices_dip: int = 1
    # Priority of the low-rank stream (torch.cuda.Stream priority: 0 = default, negative = higher).
    # Beside the DIP, the sparse-coding kernel's resident workgroups can hold off a 1024-thread
    # BatchNorm workgroup of the DIP for milliseconds; a higher-priority queue asks the dispatcher to
    # place the DIP's workgroups first.  Measured at configs[2] (bench.py --lowrank-priority, 2
    # alternating rounds): 0 -> 7.43 / 7.43 outer it/s, -1 -> 7.48 / 7.41: no effect, so 0.
    lowrank_priority: int = 0
    # Order of the sparse coding and the DIP training (lowrank='dip'): "beside" runs the
    # sparse-coding kernel concurrently with the DIP's first steps; "before" makes the DIP's stream
    # wait for it (the kernel then has the chip to itself).
    ista_dip_order: str = "beside"
    # Sparse coding on per-pattern masked Grams (lrs_ista_pat_f32: the blocks grouped by observation
    # pattern, 2 K^2 instead of 4 n K FLOP per block and iteration): "auto" when the library's cost
    # model prefers it (few patterns, n > K / 2), "on" whenever the block length allows it, "off".
    ista_patterns: str = "auto"
    # Sparse-coding iteration: "off", the reference's ISTA, or "fista", the same gradient step and prox
    # with Nesterov momentum (lrs_ista_opts.accel), on whichever path the solver picks.  An accelerated
    # call restarts its momentum, so slices of one are not one call: refused with ista_slices_dip > 1.
    ista_accel: str = "off"
    # D="learn": the lrspnp.dictlearn.DictLearnConfig of the training run (None: its defaults); bb and
    # lambda_ista are always this config's own
    dict_cfg: object = None

    @staticmethod
    def dip_1lip(**kw) -> "LrsPnPConfig":
        """Parameters of main_LRS_PnP_DIP_1-LiP.py:316-345: fro4 ISTA (Nit 100), mu1 = mu2 = 0.1,
        and the 1-Lipschitz U-Net DIP as the low-rank prox."""
        base = dict(gamma=0.5, mu1=0.1, mu2=0.1, lambda_ista=0.1, Nit=100, bb=36, sliding=36, variant="fro4",
                    lowrank="dip")
        base.update(kw)
        return LrsPnPConfig(**base)

    @staticmethod
    def dip_pro(**kw) -> "LrsPnPConfig":
        """main_LRS_PnP_DIP_pro.py:324-353: as dip_1lip, with the skip() network (5 scales of 128
        channels, 128-channel skips, plain BatchNorm, Sigmoid) as the DIP prox (:215-221)."""
        from .dip import DipConfig
        dip = kw.pop("dip", None) or DipConfig(net="skip")
        if dip.net != "skip":
            raise LrsError("dip_pro uses the skip network")
        base = dict(gamma=0.5, mu1=0.1, mu2=0.1, lambda_ista=0.1, Nit=100, bb=36, sliding=36, variant="fro4",
                    lowrank="dip", dip=dip)
        base.update(kw)
        return LrsPnPConfig(**base)

    @staticmethod
    def dip_decoder(**kw) -> "LrsPnPConfig":
        """As dip_1lip, with the Deep Decoder (include/decoder.py decodernw) as the DIP prox, trained as
        include/fit.py trains it: Adam at learning rate 0.01 for a fixed number of steps (the net is
        under-parameterised: no stopping rule), from a fixed noise input."""
        from .dip import DipConfig
        dip = kw.pop("dip", None) or DipConfig(net="decoder", learning_rate=0.01, early_stop=False)
        if dip.net != "decoder":
            raise LrsError("dip_decoder uses the decoder network")
        base = dict(gamma=0.5, mu1=0.1, mu2=0.1, lambda_ista=0.1, Nit=100, bb=36, sliding=36, variant="fro4",
                    lowrank="dip", dip=dip)
        base.update(kw)
        return LrsPnPConfig(**base)


_ALPHA = {"spec2": ops.ALPHA_SPEC2, "fro4": ops.ALPHA_FRO4, "soft": ops.ALPHA_SOFT, "matlab": ops.ALPHA_SPEC2}
_PROX = {"spec2": ops.PROX_NLM, "fro4": ops.PROX_NLM, "soft": ops.PROX_SOFT, "matlab": ops.PROX_NLM_MATLAB}
# LrsPnPConfig.svt_wide_solver -> (wide_tri, wide_mw) of the SVT calls
_SVT_WIDE_SOLVER = {"jacobi": (False, False), "tri": (True, False), "tri-mw": (True, True)}
# LrsPnPConfig's mode strings and their values: LrsPnP.__init__ checks every one before any device work
_MODES = {"variant": tuple(_PROX), "lowrank": ("svt", "dip", "tv", "nlm"), "svt_method": ("tri", "jacobi"),
          "svt_multi_wg": ("auto", "on", "off"), "svt_wide_solver": tuple(_SVT_WIDE_SOLVER),
          "ista_patterns": ("auto", "on", "off"), "ista_dip_order": ("beside", "before"),
          "ista_accel": ("off", "fista")}


# columns of LrsPnP.run()'s history: the three scores of ops.cube_quality, then LrsPnP.norms of the iteration
HISTORY_COLUMNS = ("mpsnr", "sam_deg", "rel_err", "norm_dX", "norm_dL1", "norm_dL2")


def _check_mode(name, value):
    if value not in _MODES[name]:
        raise LrsError(f"unknown {name} {value!r} ({' | '.join(_MODES[name])})")


def svt_wide_solver_flags(name):
    """(wide_tri, wide_mw) for a value of LrsPnPConfig.svt_wide_solver (host-only)."""
    _check_mode("svt_wide_solver", name)
    return _SVT_WIDE_SOLVER[name]


class LrsPnP:
    """LRS-PnP solver state on the current ROCm device.

    Y: observed unfolded cube (P x B, zeros at missing entries), M: mask (P x B), D: n x K
    dictionary with n = bb*bb.  All float32 (numpy or torch); copied to the device once.
    """

    def __init__(self, Y, M, D, cfg: LrsPnPConfig | None = None, device="cuda", image_shape=None, comm=None,
                 dip_engine: bool = True):
        """dip_engine=False (lowrank='dip' only): keep the DIP's target / mask / U buffers but build
        no network engine -- a task-parallel worker rank that never trains the DIP
        (lrspnp.dist.DipTaskSplit)."""
        self.cfg = cfg = cfg or LrsPnPConfig()
        for name in _MODES:   # every mode string, before anything is copied or enqueued
            _check_mode(name, getattr(cfg, name))
        if cfg.ista_accel != "off" and int(cfg.ista_slices_dip) > 1:
            raise LrsError("ista_accel='fista' with ista_slices_dip > 1: every accelerated call restarts its "
                           "momentum, so the slices would not be one call")
        if comm is not None and (cfg.lowrank != "svt" or cfg.svt_method != "tri"):
            raise LrsError("a row-slab shard needs lowrank='svt' with svt_method='tri'")
        if cfg.lowrank == "nlm":
            (cfg.nlm or NlmCubeConfig()).check()
        # comm: None (whole cube here) or a row-slab communicator (lrspnp.dist.SlabComm): Y, M are
        # then this rank's pixel-row slab and the SVT Gram / convergence sums are all-reduced
        self.comm = comm
        dev = torch.device(device)
        f = lambda a: torch.as_tensor(np.asarray(a, np.float32) if not isinstance(a, torch.Tensor) else a,
                                      dtype=torch.float32).to(dev).contiguous()
        self.Y, self.M = f(Y), f(M)
        self.dict_history = None
        if isinstance(D, str):
            # the dictionary learned from this solver's own observation (lrspnp.dictlearn)
            if D != "learn":
                raise LrsError(f"D must be an n x K array or 'learn', got {D!r}")
            from dataclasses import replace
            from .dictlearn import DictLearnConfig, learn_dictionary
            dcfg = replace(cfg.dict_cfg or DictLearnConfig(), bb=cfg.bb, lambda_ista=cfg.lambda_ista)
            D, self.dict_history = learn_dictionary(self.Y, self.M, dcfg, device=dev)
        self.D = f(D)
        self.P, self.B = self.Y.shape
        wide = cfg.lowrank == "svt" and self.B > 256
        if wide:
            if self.B > ops.svt_max_bands():
                raise LrsError(f"lowrank='svt' takes at most {ops.svt_max_bands()} bands, got {self.B}")
            if comm is not None:
                raise LrsError(f"a row-slab shard's SVT takes at most 256 bands, got {self.B}: the 256-band limit "
                               "of sharded SVT (lrs_svt_gram_offset)")
            if cfg.svt_multi_wg == "on":
                raise LrsError(f"svt_multi_wg='on' needs at most 256 bands, got {self.B}")
        # The SVT's solver, resolved once: the keywords of ops.svt_gram; those of ops.svt / ops.svt_finish, which add
        # the many-workgroup tridiagonal chain ("auto": on a row-slab shard); whether the sparse coding waits for
        # the Gram (above 256 bands as for svt_method='jacobi': the default eigen stage there is the warm-started
        # Jacobi chain, whose warm-start products read the Gram inside svt_gram(), so no all-reduce in between)
        wide_tri, wide_mw = svt_wide_solver_flags(cfg.svt_wide_solver)
        self._svt_gram_kw = dict(method=cfg.svt_method, wide_tri=wide and wide_tri, wide_mw=wide and wide_mw)
        self._svt_kw = dict(self._svt_gram_kw, multi_wg=cfg.svt_multi_wg == "on" or (
            cfg.svt_multi_wg == "auto" and comm is not None))
        self._gram_gates = cfg.svt_gram_first or cfg.svt_method == "jacobi" or wide
        if cfg.lowrank != "svt":
            if image_shape is None:
                raise LrsError(f"lowrank={cfg.lowrank!r} needs image_shape=(H, W) with H*W = P")
            self.H, self.W = (int(v) for v in image_shape)
            if self.H * self.W != self.P:
                raise LrsError(f"image_shape {self.H}x{self.W} does not match P = {self.P}")
        n, self.K = self.D.shape
        if n != cfg.bb * cfg.bb:
            raise LrsError(f"dictionary has {n} rows, expected bb*bb = {cfg.bb * cfg.bb}")
        self.n = n
        self.n_pad = -(-n // 16) * 16
        f32 = np.float32
        self.gamma32, self.mu1_32, self.mu2_32 = f32(cfg.gamma), f32(cfg.mu1), f32(cfg.mu2)
        self.c2 = f32(1 / cfg.mu2)                        # (1/mu_2)*lambda_2   main_LRS_PnP.py:315
        self.tau = float(f32(1 / cfg.mu2))                # SVT threshold (float32 in numpy)
        self.prox = _PROX[cfg.variant]

        # ---- block grid (host bookkeeping) -------------------------------------------------
        rows, cols = ops.block_grid(self.P, self.B, cfg.bb, cfg.sliding)
        self.nb = rows.size
        rstarts = np.unique(rows).astype(np.int32)
        cstarts = np.unique(cols).astype(np.int32)
        self.nbr = rstarts.size
        assert np.array_equal(rows, np.tile(rstarts, cstarts.size))
        assert np.array_equal(cols, np.repeat(cstarts, rstarts.size))
        rlo, rhi = ops.cover_ranges(self.P, cfg.bb, rstarts)
        clo, chi = ops.cover_ranges(self.B, cfg.bb, cstarts)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.rows_d, self.cols_d = t(rows), t(cols)
        self.grid = dict(rstarts=t(rstarts), cstarts=t(cstarts), nbr=self.nbr, rlo=t(rlo), rhi=t(rhi),
                         clo=t(clo), chi=t(chi))

        # ---- observation masks of blocks_copy (main_LRS_PnP.py:244,278) and alpha/h --------
        _, obs = ops.im2col(self.Y, None, 1.0, cfg.bb, self.rows_d, self.cols_d, self.n_pad, want_obs=True)
        self.obs = obs
        packed = np.packbits(obs.cpu().numpy(), axis=1)
        uniq, inv = np.unique(packed, axis=0, return_inverse=True)
        self.npat = uniq.shape[0]
        obs_pat = t(np.unpackbits(uniq, axis=1)[:, : self.n_pad].astype(np.uint8))
        alpha_pat, thr_pat = ops.ista_alpha(self.D, obs_pat, n, _ALPHA[cfg.variant], cfg.lambda_ista)
        inv_d = t(inv.reshape(-1).astype(np.int64))
        self.alpha = alpha_pat.index_select(0, inv_d).contiguous()
        self.thr = thr_pat.index_select(0, inv_d).contiguous()
        self.alpha_pat, self.thr_pat, self.obs_pat = alpha_pat, thr_pat, obs_pat
        self.pat_plan = None
        if self.K <= 512 and (cfg.ista_patterns == "on" or (
                cfg.ista_patterns == "auto" and ops.ista_pat_preferred(n, self.K, self.nb, self.npat, cfg.Nit))):
            plan, self.pat_ntiles = ops.ista_pat_plan(inv.reshape(-1), self.npat)
            self.pat_plan = t(plan)

        # ---- state and buffers -------------------------------------------------------------
        self.X = self.Y.clone()                           # X = Y_observed     main_LRS_PnP.py:229
        self.L1 = torch.zeros_like(self.Y)
        self.L2 = torch.zeros_like(self.Y)
        self.U = torch.empty_like(self.Y)
        self.Yb = torch.empty((self.nb, self.n_pad), dtype=torch.float32, device=dev)
        self.phi = torch.empty((self.nb, self.n_pad), dtype=torch.float32, device=dev)
        if self.pat_plan is not None:   # the dictionary and Gram images, once per solve (D, patterns fixed)
            self.ista_ws = ops.ista_pat_prepare(self.D, self.obs_pat, n)
        else:
            self.ista_ws = ops.ista_workspace(n, self.K, self.prox, dev, accel=cfg.ista_accel)
        self.norms = torch.zeros(3, dtype=torch.float64, device=dev)
        self.lowrank_stream = torch.cuda.Stream(device=dev, priority=int(cfg.lowrank_priority))
        self.iteration = 0
        self.dip = None
        self._rs_ws = self._coefs = None   # made by the first call that needs one (sparse_coding_range; sliced step)
        # beside the DIP training the sparse coding may be narrowed, or (row-split kernel: warm start) sliced
        dip, rs = cfg.lowrank == "dip", self.n_pad > 64 and self.K <= 512
        self._max_wg = cfg.ista_max_wg_dip if dip else 0
        self._slices = max(1, min(int(cfg.ista_slices_dip), cfg.Nit)) if dip and rs else 1
        if cfg.lowrank == "svt":
            self.svt_ws = ops.svt_workspace(self.P, self.B, dev)
            self.gram = ops.svt_gram_view(self.svt_ws, self.P, self.B) if comm is not None else None
        elif dip:
            self._init_dip(dev, engine=dip_engine)
        elif cfg.lowrank == "tv":
            self.tv = cfg.tv or TvProxConfig()
            self.tv_ws = ops.tvprox_workspace(self.H, self.W, self.B, dev)
        else:
            self.nlm = cfg.nlm or NlmCubeConfig()
            self.nlm_ws = ops.nlmcube_workspace(self.H, self.W, self.B, self.nlm.patch_size, self.nlm.patch_distance, dev)

    def _init_dip(self, dev, engine=True):
        """DIP target = the observed cube as an image, mask_bkg = the pixel mask
        (…1-LiP.py:275-301); the network is re-initialised every outer iteration (:214)."""
        from .dip import DipConfig, LipschitzDip, dip_nodes, frame_for
        H, W = self.H, self.W
        dcfg = self.cfg.dip or DipConfig()
        self.dip = LipschitzDip(self.B, H, W, dcfg, device=dev,
                                 stream_priority=self.cfg.lowrank_priority) if engine else None
        # An image of a size the net does not reproduce lives inside a reflected frame (dip.frame_for): the
        # target and the net input are written framed, (B, Hf, Wf); the mask stays the image's (DipProx
        # frames it once, zeros outside).  Without an engine (a DipTaskSplit worker) the frame is still
        # worked out on the host, so every rank holds the same buffers.
        if self.dip is not None:
            self.frame = (self.dip.Hf, self.dip.Wf, self.dip.top, self.dip.left)
        elif dcfg.frame == "auto":
            self.frame = frame_for(dip_nodes(dcfg, self.B), H, W)
        else:
            self.frame = (H, W, 0, 0)
        Hf, Wf, top, left = self.frame
        self.framed = (Hf, Wf) != (H, W)
        self.dip_target = torch.empty((self.B, Hf, Wf), dtype=torch.float32, device=dev)
        if self.framed:
            ops.unfolded_to_frame(self.Y, None, 1.0, H, W, top, left, Hf, Wf, self.dip_target)
        else:
            ops.unfolded_to_image(self.Y, None, 1.0, H, W, self.dip_target)
        # The reference's mask_bkg is one (1,1,H,W) pixel mask.  A mask M that differs between bands
        # (dead columns, dropped lines, missing bands) goes to the loss per element instead, as
        # (B, H, W): the mask the caller passed is the specification (one device check, here only).
        if bool((self.M == self.M[:, :1]).all()):
            pix = ops.unfolded_to_image(self.M[:, :1].contiguous(), None, 1.0, H, W)   # (1, H, W)
            self.dip_mask = pix.reshape(-1).contiguous()
        else:
            self.dip_mask = ops.unfolded_to_image(self.M, None, 1.0, H, W)             # (B, H, W)
        # (the decoder's input is its own fixed noise, DipProx.decoder_input: no image is written for it)
        self.dip_in = None if dcfg.net == "decoder" else torch.empty_like(self.dip_target)
        self.dip_steps = []

    # -----------------------------------------------------------------------------------------
    def sparse_coding(self, stream=None, want_coefs=False):
        """Yb = blocks of X + L1/mu1; Phi = D * ISTA-PnP(Yb) for every block."""
        self._im2col(stream)
        return self._ista(self.cfg.Nit, stream, want_coefs=want_coefs)

    def _im2col(self, stream, blocks=slice(None)):
        ops.im2col(self.X, self.L1, self.mu1_32, self.cfg.bb, self.rows_d[blocks], self.cols_d[blocks], self.n_pad,
                   Yb=self.Yb[blocks], stream=stream)

    def _ista(self, Nit, stream, want_coefs=False, coefs=None, warm_start=False, max_workgroups=0):
        """All blocks' ISTA into self.phi: the per-pattern Gram path when planned, else lrs_ista_f32."""
        if self.pat_plan is not None:
            return ops.ista_pat(self.Yb, self.obs_pat, self.pat_plan, self.pat_ntiles, self.K, self.n, self.alpha,
                                self.thr, Nit, self.ista_ws, self.prox, phi=self.phi, coefs=coefs,
                                want_coefs=want_coefs, stream=stream, max_workgroups=max_workgroups,
                                warm_start=warm_start, accel=self.cfg.ista_accel)
        return ops.ista(self.Yb, self.obs, self.D, self.n, self.alpha, self.thr, Nit, self.prox, phi=self.phi,
                        coefs=coefs, want_coefs=want_coefs, ws=self.ista_ws, stream=stream,
                        max_workgroups=max_workgroups, warm_start=warm_start, accel=self.cfg.ista_accel)

    def sparse_coding_range(self, b0: int, b1: int, stream=None):
        """Phi rows [b0, b1) only (the blocks of one task-parallel worker, lrspnp.dist.DipTaskSplit)."""
        if b1 <= b0:
            return
        self._im2col(stream, slice(b0, b1))
        ws = self.ista_ws
        if self.pat_plan is not None:   # a block range runs the row-split kernel, on a workspace of its own
            if self._rs_ws is None:
                self._rs_ws = ops.ista_workspace(self.n, self.K, self.prox, self.Yb.device, accel=self.cfg.ista_accel)
            ws = self._rs_ws
        ops.ista(self.Yb[b0:b1], self.obs[b0:b1], self.D, self.n, self.alpha[b0:b1], self.thr[b0:b1], self.cfg.Nit,
                 self.prox, phi=self.phi[b0:b1], ws=ws, stream=stream, accel=self.cfg.ista_accel)

    def admm(self, stream=None):
        """col2im + closed-form X + dual updates from the current Phi and U (main_LRS_PnP.py:324-366)."""
        ops.admm_update(self.X, self.L1, self.L2, self.Y, self.M, self.U, self.phi, self.cfg.bb, self.grid,
                        self.gamma32, self.mu1_32, self.mu2_32, norms=self.norms,
                        stream=stream or torch.cuda.current_stream())
        self.iteration += 1

    def low_rank_tv(self, stream=None, stats=None):
        """U = prox_{tau T}(X + L2/mu2), tau = 1/mu2 as the SVT's, on `stream` (ops.tvprox)."""
        tv = self.tv
        return ops.tvprox(self.X, self.L2, self.c2, self.H, self.W, self.tv_ws, U=self.U, w_sp=tv.w_sp, w_bd=tv.w_bd,
                          w_ss=tv.w_ss, tau=self.tau, n_iter=tv.n_iter, warm=tv.warm and self.iteration > 0,
                          stats=stats, stream=stream)

    def low_rank_nlm(self, stream=None):
        """U = NLM(X + L2/mu2) on `stream` (ops.nlmcube); h and sigma are the config's own, not 1/mu2."""
        c = self.nlm
        return ops.nlmcube(self.X, self.L2, self.c2, self.H, self.W, self.nlm_ws, U=self.U, patch_size=c.patch_size,
                           patch_distance=c.patch_distance, h=c.h, sigma=c.sigma, stream=stream)

    def _svt_warm(self):
        return self.cfg.svt_warm and self.iteration > 0

    def low_rank(self, stream=None, s_out=None):
        return ops.svt(self.X, self.L2, self.c2, self.tau, self.svt_ws, U=self.U, s_out=s_out, warm=self._svt_warm(),
                       stream=stream, **self._svt_kw)

    def low_rank_dip(self, stream):
        """U = DIP(X + L2/mu2) (…1-LiP.py:399-411) on `stream`; the host polls early stopping."""
        Hf, Wf, top, left = self.frame
        if self.dip_in is None:
            pass
        elif self.framed:
            ops.unfolded_to_frame(self.X, self.L2, self.c2, self.H, self.W, top, left, Hf, Wf, self.dip_in,
                                  stream=stream)
        else:
            ops.unfolded_to_image(self.X, self.L2, self.c2, self.H, self.W, self.dip_in, stream=stream)
        with torch.cuda.stream(stream):
            img = self.dip.run(self.dip_target, self.dip_in, self.dip_mask, seed=self.cfg.dip_seed + self.iteration,
                               early_stop=self.dip.cfg.early_stop)
            if self.dip.last_framed is not None:   # a fixed-step run inside a frame: the image out of the framed output
                ops.frame_to_unfolded(self.dip.last_framed, self.H, self.W, top, left, self.U, stream=stream)
            else:
                ops.image_to_unfolded(img, self.H, self.W, self.U, stream=stream)
        self.dip_steps.append((self.dip.last_steps, self.dip.last_stop_epoch))

    # The per-mode parts of step(): early(lr) is enqueued before im2col and may return an event the sparse
    # coding waits for; late(main, lr) is enqueued after the sparse coding.
    def _svt_early(self, lr):
        warm = self._svt_warm()   # first half (whole chip, ~0.2 ms): fp64 Gram (+ Jacobi warm-start products)
        ops.svt_gram(self.X, self.L2, self.c2, self.svt_ws, warm=warm, stream=lr, **self._svt_gram_kw)
        if self.comm is not None:
            self.comm.allreduce_(self.gram, lr)       # the cube's Gram = sum of the slabs' Grams
        gram_done = lr.record_event()
        # second half: the one-workgroup eigensolver then runs beside the sparse coding
        ops.svt_finish(self.X, self.L2, self.c2, self.tau, self.svt_ws, self.U, warm=warm, stream=lr, **self._svt_kw)
        # gated: the Gram gets the chip before the sparse coding fills it, so the ~7 ms Jacobi solve starts at once;
        # the tridiagonal chain fits inside the sparse coding even when its Gram waits for workgroups to retire
        return gram_done if self._gram_gates else None

    def _tv_early(self, lr):
        self.low_rank_tv(lr)   # the stencil passes run beside im2col and the sparse coding; no host sync

    def _dip_late(self, main, lr):
        # the sparse coding was enqueued first, so it runs beside the DIP training unless the order says
        if self.cfg.ista_dip_order == "before":
            stream_wait(lr, main)
        self.low_rank_dip(lr)

    def _nlm_early(self, lr):
        self.low_rank_nlm(lr)   # the one launch runs beside im2col and the sparse coding; no host sync

    _PARTS = {"svt": (_svt_early, None), "tv": (_tv_early, None), "nlm": (_nlm_early, None), "dip": (None, _dip_late)}

    def step(self):
        """One outer ADMM iteration (main_LRS_PnP.py:250-366), stream-ordered.  No host sync in
        the SVT and TV modes; the DIP mode polls its early-stopping flag on the low-rank stream only."""
        if self.cfg.lowrank == "dip" and self.dip is None:
            raise LrsError("this LrsPnP was built without a DIP engine (dip_engine=False)")
        early, late = self._PARTS[self.cfg.lowrank]
        main, lr = torch.cuda.current_stream(), self.lowrank_stream
        stream_wait(lr, main)
        gate = early(self, lr) if early else None
        self._im2col(main)
        if gate is not None:
            main.wait_event(gate)
        Nit, sl = self.cfg.Nit, self._slices
        if sl > 1 and self._coefs is None:
            self._coefs = torch.empty((self.nb, self.K), dtype=torch.float32, device=self.Yb.device)
        for k in range(sl):   # beside the DIP, Nit may be split over launches that continue from the coefficients
            self._ista(Nit * (k + 1) // sl - Nit * k // sl, main, coefs=self._coefs, want_coefs=sl > 1,
                       warm_start=k > 0, max_workgroups=self._max_wg)
        if late:
            late(self, main, lr)
        stream_wait(main, lr)
        self.admm(main)

    def _unfolded(self, a, what):
        """a as a contiguous float32 (P, B) device tensor: unfolded (P, B) as it is, an image (B, H, W) through
        ops.image_to_unfolded."""
        a = torch.as_tensor(a if isinstance(a, torch.Tensor) else np.asarray(a, np.float32), dtype=torch.float32)
        a = a.to(self.Y.device).contiguous()
        if a.dim() == 3 and a.shape[0] == self.B and a.shape[1] * a.shape[2] == self.P:
            return ops.image_to_unfolded(a, a.shape[1], a.shape[2])
        if tuple(a.shape) != (self.P, self.B):
            raise LrsError(f"{what} must be (B, H, W) with H*W = {self.P}, B = {self.B}, or unfolded "
                           f"({self.P}, {self.B}); got {tuple(a.shape)}")
        return a

    def run(self, n_iter, clean=None, region="all", keep_best=None):
        """n_iter outer iterations (step()), each scored on the device against `clean`, and the best iterate
        kept there: the loop of the reference mains (main_LRS_PnP.py:368-391: MPSNR after every iteration,
        best_PSNR) without a host sync per iteration.

        clean: the clean cube, (B, H, W) or unfolded (P, B); None records the convergence columns only.
        region: "all", "hole" (the entries with M == 0) or an array like clean, nonzero = scored.
        keep_best: None, or the score whose best iterate is kept: "mpsnr" (largest), "rel_err" or "sam" (smallest).
        Per iteration, on the current stream after step(): ops.cube_quality, ops.keep_best, and the copy of the
        three scores and of self.norms into row t of a device history.  One read at the end.  Returns the
        history, a numpy record array of n_iter rows with the columns HISTORY_COLUMNS (norm_* are self.norms:
        the squared norms convergence() takes the log-root of; the score columns are NaN without clean).  With
        keep_best, self.best_X is that iterate (a device tensor), self.best_iteration its row in the history (the
        first of equals) and self.best_score its score; None when no iteration had a score that is not NaN."""
        n_iter = int(n_iter)
        if n_iter < 1:
            raise LrsError(f"run() needs n_iter >= 1, got {n_iter}")
        if self.comm is not None:
            raise LrsError("run() does not serve a row-slab shard (comm): its scores would be the slab's alone")
        if keep_best is not None and keep_best not in self._KEEP:
            raise LrsError(f"unknown keep_best {keep_best!r} ({' | '.join(self._KEEP)} | None)")
        if clean is None and keep_best is not None:
            raise LrsError(f"keep_best={keep_best!r} needs the clean cube: there is no score without it")
        if isinstance(region, str) and region not in ("all", "hole"):
            raise LrsError(f"unknown region {region!r} (all | hole | an array)")
        dev = self.Y.device
        # the history rows and, behind them, keep_best's {score, iteration}: one buffer, one read at the end
        rec = torch.full((n_iter * 6 + 2,), float("nan"), dtype=torch.float64, device=dev)
        hist = rec[: n_iter * 6].view(n_iter, 6)
        q = best = None
        if clean is not None:
            C = self._unfolded(clean, "clean")
            if isinstance(region, str):
                reg = None if region == "all" else (self.M == 0).to(torch.uint8)
            else:
                reg = (self._unfolded(region, "region") != 0).to(torch.uint8)
            ws = ops.cube_quality_workspace(self.P, self.B, dev)
            q = torch.empty(4, dtype=torch.float64, device=dev)
            if keep_best is not None:
                col, sign = self._KEEP[keep_best]
                self.best_X = torch.empty_like(self.X)
                best = rec[n_iter * 6:]
        self.best_iteration = self.best_score = None
        if best is None:
            self.best_X = None
        for t in range(n_iter):
            self.step()
            if q is not None:
                ops.cube_quality(self.X, C, reg, ws=ws, q=q)
                if best is not None:
                    ops.keep_best(q[col:col + 1], sign, t, self.X, self.best_X, best)
                hist[t, :3].copy_(q[:3])
            hist[t, 3:].copy_(self.norms)
        h = rec.cpu().numpy()   # the one read
        h, (score, it) = h[: n_iter * 6].reshape(n_iter, 6), h[n_iter * 6:].tolist()
        if best is not None:
            if score == score:
                self.best_score, self.best_iteration = score, int(it)
            else:
                self.best_X = None
        return np.rec.fromarrays(h.T, names=list(HISTORY_COLUMNS))

    # keep_best -> (index in q, sign): the largest MPSNR, the smallest SAM or relative error
    _KEEP = {"mpsnr": (0, 1), "sam": (1, -1), "rel_err": (2, -1)}

    def convergence(self):
        """state_convergence (main_LRS_PnP.py:23-25) of X, lambda_1, lambda_2 for the last step."""
        norms = self.norms
        if self.comm is not None:
            norms = norms.clone()
            self.comm.allreduce_(norms, torch.cuda.current_stream())
        return torch.log(torch.sqrt(norms)).cpu().tolist()

"""ctypes binding of liblrspnp_hip.so (include/lrspnp.h).

The product path has no CPU fallback: if the library is missing, fails to load, or the device is
not gfx950, every op raises ``LrsError`` instead of computing anything elsewhere.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# LRSPNP_LIB: another build of the same library (A/B timing of kernel variants: tools/gpu.sh steptime)
LIB_PATH = os.environ.get("LRSPNP_LIB") or os.path.join(_HERE, "liblrspnp_hip.so")
CSRC = os.path.join(os.path.dirname(_HERE), "csrc")

LRS_OK = 0
LRS_E = {-1: "LRS_E_INVALID", -2: "LRS_E_UNSUPPORTED", -3: "LRS_E_WORKSPACE", -4: "LRS_E_NODEVICE"}

ALPHA_SPEC2, ALPHA_FRO4, ALPHA_SOFT = 0, 1, 2
PROX_NLM, PROX_SOFT, PROX_NLM_MATLAB = 0, 1, 2


class LrsError(RuntimeError):
    pass


# per-call / per-handle options (include/lrspnp.h); the library keeps no process-wide mode
ISTA_F32, ISTA_SPLIT_BF16 = 0, 1
DIP_F32, DIP_SPLIT_BF16 = 0, 1


ISTA_ALGO_AUTO, ISTA_ALGO_GENERIC = 0, 1
ISTA_ACCEL_NONE, ISTA_ACCEL_FISTA = 0, 1
ISTA_ACCEL = {"off": ISTA_ACCEL_NONE, "fista": ISTA_ACCEL_FISTA}

# flag word (`warm`) of the SVT calls
SVT_WARM, SVT_JACOBI, SVT_MULTI_WG, SVT_WIDE_TRI, SVT_WIDE_MW = 1, 2, 4, 8, 16
# flag word of lrs_tvprox_f32
TVPROX_WARM = 1


class IstaOpts(ctypes.Structure):
    _fields_ = [("precision", ctypes.c_int32), ("max_workgroups", ctypes.c_int32), ("algorithm", ctypes.c_int32),
                ("warm_start", ctypes.c_int32), ("accel", ctypes.c_int32), ("reserved", ctypes.c_int32 * 3)]


class DipOpts(ctypes.Structure):
    _fields_ = [("precision", ctypes.c_int32), ("upsample_dgrad", ctypes.c_int32), ("reserved", ctypes.c_int32 * 6)]


def ista_opts(precision: int = ISTA_SPLIT_BF16, max_workgroups: int = 0, algorithm: int = ISTA_ALGO_AUTO,
              warm_start: int = 0, accel: int = ISTA_ACCEL_NONE) -> IstaOpts:
    return IstaOpts(precision=precision, max_workgroups=max_workgroups, algorithm=algorithm, warm_start=warm_start,
                    accel=accel)


def ista_accel(name) -> int:
    """lrs_ista_opts.accel for "off" | "fista" (anything else is refused here, before any call)."""
    if name not in ISTA_ACCEL:
        raise LrsError(f"unknown accel {name!r} ({' | '.join(ISTA_ACCEL)})")
    return ISTA_ACCEL[name]


def dip_opts(precision: int = DIP_SPLIT_BF16, upsample_dgrad: int = 0) -> DipOpts:
    return DipOpts(precision=precision, upsample_dgrad=upsample_dgrad)


_lib = None
_device_checked = False


def build(force: bool = False) -> str:
    """Compile csrc/ for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    import subprocess

    if force:
        subprocess.check_call(["make", "-s", "-C", CSRC, "clean"])
    subprocess.check_call(["make", "-s", "-j8", "-C", CSRC])
    return LIB_PATH


def _declare(L):
    c = ctypes
    vp, i64, i32, f32, f64, sz = c.c_void_p, c.c_int64, c.c_int, c.c_float, c.c_double, c.c_size_t
    i32p = c.POINTER(c.c_int32)
    dop = c.POINTER(DipOpts)
    sig = {
        "lrs_version": (c.c_char_p, []),
        "lrs_check_device": (i32, []),
        "lrs_nlm_col_f32": (i32, [vp, i64, vp, i64, i64, i64, f64, vp, i32, i32, vp]),
        "lrs_block_count": (i64, [i64, i64, i64, i64]),
        "lrs_block_grid": (i32, [i64, i64, i64, i64, i32p, i32p, i64]),
        "lrs_cover_ranges": (i32, [i64, i64, i32p, i64, i32p, i32p]),
        "lrs_im2col_f32": (i32, [vp, vp, f32, i64, i64, i64, vp, vp, i64, i64, vp, vp, vp]),
        "lrs_ista_alpha_workspace": (sz, [i64, i64, i64]),
        "lrs_ista_alpha_f32": (i32, [vp, i64, i64, vp, i64, i64, i32, f32, vp, vp, vp, sz, vp]),
        "lrs_ista_workspace": (sz, [i64, i64, i32, c.POINTER(IstaOpts)]),
        "lrs_ista_f32": (i32, [vp, vp, vp, i64, i64, i64, i64, vp, vp, i32, i32, vp, vp, c.POINTER(IstaOpts), vp,
                               sz, vp]),
        "lrs_nlm_matlab_col_f32": (i32, [vp, i64, vp, i64, i64, i64, f64, vp, vp]),
        "lrs_ista_pat_plan_len": (i64, [i64, i64]),
        "lrs_ista_pat_plan": (i64, [i32p, i64, i64, i32p, i64]),
        "lrs_ista_pat_preferred": (i32, [i64, i64, i64, i64, i32]),
        "lrs_ista_pat_workspace": (sz, [i64, i64, i64]),
        "lrs_ista_pat_prepare": (i32, [vp, i64, i64, vp, i64, i64, vp, sz, vp]),
        "lrs_ista_pat_f32": (i32, [vp, vp, i64, vp, i64, i64, i64, i64, i64, vp, vp, i32, i32, vp, vp,
                                   c.POINTER(IstaOpts), vp, sz, vp]),
        "lrs_dict_workspace": (sz, [i64, i64, i64, i64]),
        "lrs_dict_stats_f32": (i32, [vp, i64, i64, vp, vp, vp, sz, vp]),
        "lrs_dict_update_f32": (i32, [vp, vp, vp, vp, i64, i64, i64, i64, vp, i32, vp, vp, sz, vp]),
        "lrs_dict_normalise_f32": (i32, [vp, i64, i64, vp]),
        "lrs_ssim_f32":(i32, [vp, vp, i32, i32, i32, vp, vp]),
        "lrs_psnr_workspace": (sz, [i64, i64]),
        "lrs_psnr_bands_f32": (i32, [vp, vp, i64, i64, vp, vp, sz, vp]),
        "lrs_cube_quality_workspace": (sz, [i64, i64]),
        "lrs_cube_quality_f32": (i32, [vp, vp, vp, i64, i64, vp, vp, vp, sz, vp]),
        "lrs_keep_best_f32": (i32, [vp, i32, c.c_int32, vp, vp, i64, vp, vp]),
        "lrs_svt_max_bands": (i64, []),
        "lrs_svt_workspace": (sz, [i64, i64]),
        "lrs_svt_f32": (i32, [vp, vp, f32, i64, i64, f64, vp, vp, i32, vp, sz, vp]),
        "lrs_svt_gram_f32": (i32, [vp, vp, f32, i64, i64, i32, vp, sz, vp]),
        "lrs_svt_finish_f32": (i32, [vp, vp, f32, i64, i64, f64, vp, vp, i32, vp, sz, vp]),
        "lrs_svt_gram_offset": (i32, [i64, i64, vp, vp]),
        "lrs_diag_svt_state": (i32, [vp, i64, i64, vp]),
        "lrs_diag_svt_plan": (i32, [i64, i32, i32p]),
        "lrs_diag_svt_apply": (i32, [vp, vp, f32, i64, i64, vp, vp, vp]),
        "lrs_tvprox_workspace": (sz, [i64, i64, i64]),
        "lrs_tvprox_f32": (i32, [vp, vp, f32, i64, i64, i64, f32, f32, f32, f64, i32, i32, vp, vp, vp, sz, vp]),
        "lrs_nlmcube_workspace": (sz, [i64, i64, i64, i32, i32]),
        "lrs_nlmcube_f32": (i32, [vp, vp, f32, i64, i64, i64, i32, i32, f64, f64, vp, vp, sz, vp]),
        "lrs_admm_update_f32": (i32, [vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, vp, vp, i64, vp, vp,
                                      vp, vp, f32, f32, f32, vp, vp, vp]),
        # DIP low-rank prox
        "lrs_conv2d_out_size": (i32, [i32, i32, i32, i32, i32, i32, c.POINTER(c.c_int), c.POINTER(c.c_int)]),
        "lrs_conv2d_col_size": (i64, [i32, i32, i32, i32, i32, i32, i32]),
        "lrs_conv2d_workspace": (sz, [i32, i32, i32, i32, i32, i32, i32, i32, dop]),
        "lrs_conv2d_fwd_f32": (i32, [vp, i32, i32, i32, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, dop, vp, sz,
                                     vp]),
        "lrs_conv2d_bwd_f32": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, dop, vp,
                                     sz, vp]),
        "lrs_conv2d_bwd_x_f32": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, dop, vp,
                                       sz, vp]),
        "lrs_bn_act_workspace": (sz, [i32, i64]),
        "lrs_bn_act_fwd_f32": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i64, i32, f32, f32, vp, sz, vp]),
        "lrs_bn_act_bwd_f32": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i64, i32, vp, sz, vp]),
        "lrs_conv_bn_small_f32": (i32, [vp, i32, i32, i32, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, i32, i32,
                                        vp, vp, vp, vp, vp, vp, vp]),
        "lrs_up2_bilinear_act_fwd_f32": (i32, [vp, i32, i32, i32, i32, vp, vp]),
        "lrs_up2_bilinear_act_bwd_f32": (i32, [vp, vp, i32, i32, i32, i32, vp, vp]),
        "lrs_sigma_max_workspace": (sz, [i32]),
        "lrs_sigma_max_f32": (i32, [c.POINTER(vp), c.POINTER(vp), c.POINTER(c.c_int), c.POINTER(c.c_int), i32,
                                    f32, vp, vp, vp, sz, vp]),
        "lrs_diag_sigma_phases": (i32, [c.POINTER(vp), c.POINTER(c.c_int), c.POINTER(c.c_int), i32, vp, sz, vp, vp]),
        "lrs_adam_f32": (i32, [vp, vp, vp, vp, i64, vp, f32, f32, f32, f32, vp]),
        "lrs_masked_mse_f32": (i32, [vp, vp, vp, i32, i64, vp, vp, vp]),
        "lrs_masked_mse_cmask_f32": (i32, [vp, vp, vp, i32, i32, i64, vp, vp, vp]),
        "lrs_unfolded_to_image_f32": (i32, [vp, vp, f32, i64, i64, i64, vp, vp]),
        "lrs_image_to_unfolded_f32": (i32, [vp, i64, i64, i64, vp, vp]),
        "lrs_masked_mse_framed_f32": (i32, [vp, vp, vp, i32, i32, i64, i64, vp, vp, vp]),
        "lrs_unfolded_to_frame_f32": (i32, [vp, vp, f32, i64, i64, i64, i64, i64, i64, i64, vp, vp]),
        "lrs_frame_to_unfolded_f32": (i32, [vp, i64, i64, i64, i64, i64, i64, i64, vp, vp]),
        "lrs_dipnet_set_frame": (i32, [vp, i32, i32, i32, i32]),
        "lrs_dipnet_get_frame": (i32, [vp] + [c.POINTER(c.c_int)] * 4),
        "lrs_sstv_f32": (i32, [vp, i32, i32, i32, i32, i32, i32, i32, f32, f32, f32, f32, i64, vp, vp, vp]),
        "lrs_es_ring_bytes": (sz, [i32, i64]),
        "lrs_es_init": (i32, [vp, i32, i32, vp]),
        "lrs_es_update_f32": (i32, [vp, i64, vp, vp, vp]),
        "lrs_dipnet_create": (i32, [vp, i32, i32, i32, i32, dop, c.POINTER(vp)]),
        "lrs_dipnet_get_opts": (i32, [vp, dop]),
        "lrs_dipnet_node_shape": (i32, [vp, i32, c.POINTER(c.c_int), c.POINTER(c.c_int), c.POINTER(c.c_int)]),
        "lrs_dipnet_destroy": (None, [vp]),
        "lrs_dipnet_num_params": (i64, [vp]),
        "lrs_dipnet_num_bnstats": (i64, [vp]),
        "lrs_dipnet_workspace": (sz, [vp]),
        "lrs_dipnet_param_offsets": (i32, [vp, i32, c.POINTER(i64), c.POINTER(i64), c.POINTER(i64),
                                           c.POINTER(i64)]),
        "lrs_dipnet_out_shape": (i32, [vp, c.POINTER(c.c_int), c.POINTER(c.c_int), c.POINTER(c.c_int)]),
        "lrs_dipnet_bind": (i32, [vp, vp, vp, vp, vp, vp, vp, sz]),
        "lrs_dipnet_init_params": (i32, [vp, c.c_uint64, vp]),
        "lrs_dipnet_reset_optimizer": (i32, [vp, vp]),
        "lrs_dipnet_forward": (i32, [vp, vp, vp]),
        "lrs_dipnet_backward": (i32, [vp, vp, vp, vp]),
        "lrs_dipnet_set_ln_lambda": (i32, [vp, f32]),
        "lrs_dipnet_output": (c.c_size_t, [vp]),
        "lrs_dipnet_grads": (c.c_size_t, [vp]),
        "lrs_dipnet_node_buffer": (c.c_size_t, [vp, i32, i32]),
        "lrs_dipnet_train_steps": (i32, [vp, vp, vp, vp, f32, f32, f32, f32, vp, vp, i32, i32, vp]),
        "lrs_dipnet_train_steps_cmask": (i32, [vp, vp, vp, vp, i32, f32, f32, f32, f32, vp, vp, i32, i32, vp]),
        "lrs_dipnet_last_loss": (i32, [vp, c.POINTER(f64), vp]),
        "lrs_stream_wait": (i32, [vp, vp]),
    }
    # The product library must export every row.  A variant build named by LRSPNP_LIB (A/B timing) may predate
    # some: a row it lacks is skipped, so its other paths still time against this one, and a call of a
    # skipped entry point then fails at that call (ctypes' AttributeError), not at load.
    variant = bool(os.environ.get("LRSPNP_LIB"))
    for name, (res, args) in sig.items():
        if variant and not hasattr(L, name):
            continue
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    return L


def lib():
    """The loaded library (host-side entry points usable without a GPU)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LrsError(f"{LIB_PATH} not built: run __graft_entry__.build() (make -C {CSRC})")
        try:
            _lib = _declare(ctypes.CDLL(LIB_PATH))
        except OSError as e:  # pragma: no cover - environment problem
            raise LrsError(f"cannot load {LIB_PATH}: {e}") from e
    return _lib


def device_lib():
    """The library, after checking that the current device is a gfx950 (MI355X)."""
    global _device_checked
    L = lib()
    if not _device_checked:
        import torch

        if not torch.cuda.is_available():
            raise LrsError("no ROCm GPU visible: lrspnp has no CPU fallback")
        rc = L.lrs_check_device()
        if rc != LRS_OK:
            raise LrsError(f"lrs_check_device: {LRS_E.get(rc, rc)} (need gfx950)")
        _device_checked = True
    return L


def check(rc: int, what: str) -> None:
    if rc != LRS_OK:
        raise LrsError(f"{what} failed: {LRS_E.get(rc, f'hipError {rc}')}")


# ---- what every wrapper (ops, dip, metrics) passes to the library ---------------------------------------
def ptr(t):
    """A tensor's device pointer (None stays NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def sptr(stream=None):
    """A torch stream's hipStream_t (None: the current stream)."""
    if stream is None:
        import torch

        stream = torch.cuda.current_stream()
    return ctypes.c_void_p(stream.cuda_stream)


def dev(t, dtype, name):
    """t, after checking that it is a contiguous device tensor of dtype."""
    import torch

    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise LrsError(f"{name} must be a CUDA(ROCm) tensor")
    if t.dtype != dtype:
        raise LrsError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise LrsError(f"{name} must be contiguous")
    return t


def outs(fn, what: str, *args, n: int = 3, ctype=ctypes.c_int) -> tuple:
    """fn(*args, &o_0, ..., &o_{n-1}), checked: the values of its n trailing out-parameters of ctype."""
    o = [ctype() for _ in range(n)]
    check(fn(*args, *[ctypes.byref(x) for x in o]), what)
    return tuple(x.value for x in o)


def mask_channels(mask, C: int, P: int, hw=("H", "W")) -> int:
    """The mode of a DIP loss mask for a C x P output: 1 for a pixel mask (P elements, applied to every
    channel), C for a per-element mask (C*P elements, the layout of the output: a mask that differs
    between bands); None (no mask) counts as 1.  Anything else is refused; hw: the image's (H, W) where the
    caller knows it, for that message."""
    if mask is None:
        return 1
    n = mask.numel()
    if n == P:
        return 1
    if n == C * P:
        return C
    H, W = hw
    raise LrsError(f"mask has {n} elements ({tuple(mask.shape)}): expected a pixel mask ({P},) / ({H}, {W}) or a "
                   f"per-band mask ({C}, {H}, {W})")

"""Host side of the band-varying DIP masks (no GPU): lrspnp.data.stripe_mask, the mask-mode choice
from the element count, and the refusals of the new C entry points that never reach the device
(in the style of tests/test_abi.py)."""
import ctypes

import numpy as np
import pytest

from lrspnp import _lib
from lrspnp.data import fold, stripe_mask, unfold

# (H, W, B, seed, missing_band) of every stripe_mask the GPU tests draw (tests/test_gpu_dip_bandmask.py)
GPU_MASKS = [(36, 36, 8, 3, 5), (68, 68, 8, 4, 2), (20, 20, 2, 5, 1), (36, 36, 8, 7, 6)]


def test_stripe_mask_is_seeded():
    a, b = stripe_mask(36, 36, 8, 3), stripe_mask(36, 36, 8, 3)
    assert a.dtype == np.float32 and a.shape == (8, 36, 36) and np.array_equal(a, b)
    assert not np.array_equal(a, stripe_mask(36, 36, 8, 4))
    assert set(np.unique(a).tolist()) <= {0.0, 1.0}
    # True: a seeded choice of the missing band, the same every time
    c = stripe_mask(36, 36, 8, 3, missing_band=True)
    assert np.array_equal(c, stripe_mask(36, 36, 8, 3, missing_band=True))
    assert sum(int(c[b].sum() == 0) for b in range(8)) == 1


@pytest.mark.parametrize("H,W,B,seed,mb", GPU_MASKS)
def test_stripe_mask_observed_share_and_band_variation(H, W, B, seed, mb):
    """The default parametrisation leaves 90-95 % observed (the reference mask's regime) at every shape and
    seed the GPU tests use.  A missing band is the option on top of that default: with it the share is
    taken over the other bands, which is the same figure (one of 8 bands gone is 12.5 % on its own)."""
    m = stripe_mask(H, W, B, seed)
    assert 0.90 <= float(m.mean()) <= 0.95, float(m.mean())
    assert any(not np.array_equal(m[0], m[b]) for b in range(1, B))          # at least two bands differ
    # dead columns: per band at least one wholly dead image column, not the same set in every band
    dead = [frozenset(np.flatnonzero(m[b].sum(axis=0) == 0).tolist()) for b in range(B)]
    assert all(len(d) >= 1 for d in dead) and len(set(dead)) > 1
    assert all(float(m[b][:, [j for j in range(W) if j not in dead[b]]].mean()) < 1.0 for b in range(B))   # dead pixels
    mm = stripe_mask(H, W, B, seed, missing_band=mb)
    assert float(mm[mb].sum()) == 0.0
    keep = [b for b in range(B) if b != mb]
    assert np.array_equal(mm[keep], m[keep])
    assert 0.90 <= float(mm[keep].mean()) <= 0.95


def test_stripe_mask_unfold_is_the_solver_orientation():
    """M = unfold(stripe_mask) is (P, B) with row p = i + H j: M[i + H j, b] = mask[b, i, j], the layout
    lrs_unfolded_to_image_f32 reads back into (B, H, W)."""
    H, W, B = 5, 7, 3
    m = stripe_mask(H, W, B, 1, col_frac=0.2, pixel_frac=0.1, missing_band=2)
    M = unfold(m)
    assert M.shape == (H * W, B) and M.dtype == np.float32
    for b, i, j in [(0, 0, 0), (1, 4, 6), (2, 3, 1), (0, 2, 5)]:
        assert M[i + H * j, b] == m[b, i, j]
    assert np.array_equal(fold(M, H, W), m)
    assert float(M[:, 2].sum()) == 0.0


def test_stripe_mask_refuses_bad_arguments():
    with pytest.raises(ValueError):
        stripe_mask(0, 4, 2)
    with pytest.raises(ValueError):
        stripe_mask(4, 4, 2, missing_band=2)
    with pytest.raises(ValueError):
        stripe_mask(4, 4, 2, pixel_frac=1.0)


def test_mask_channels_from_element_count():
    torch = pytest.importorskip("torch")
    from lrspnp import ops
    C, P = 8, 1296
    assert ops.mask_channels(None, C, P) == 1
    assert ops.mask_channels(torch.zeros(P), C, P) == 1
    assert ops.mask_channels(torch.zeros(36, 36), C, P) == 1
    assert ops.mask_channels(torch.zeros(C, 36, 36), C, P) == C
    assert ops.mask_channels(torch.zeros(1, 16), 1, 16) == 1          # C = 1: the two modes coincide
    for bad in (torch.zeros(C * P + 1), torch.zeros(2, 36, 36), torch.zeros(0)):
        with pytest.raises(_lib.LrsError, match=r"pixel mask.*per-band mask"):
            ops.mask_channels(bad, C, P)


def test_cmask_entry_points_refuse_bad_arguments_on_the_host():
    """Null handles / pointers and mask channel counts other than 1 or C return LRS_E_INVALID (-1) from
    checks that come before any device access."""
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)   # never dereferenced: the argument checks come first
    f = ctypes.c_float
    assert L.lrs_dipnet_train_steps_cmask(None, fake, fake, fake, 1, f(0.1), f(0.9), f(0.999), f(1e-8), None, None,
                                          1, 0, None) == -1
    assert L.lrs_masked_mse_cmask_f32(None, fake, fake, 1, 8, 64, None, fake, None) == -1
    assert L.lrs_masked_mse_cmask_f32(fake, None, fake, 1, 8, 64, None, fake, None) == -1
    assert L.lrs_masked_mse_cmask_f32(fake, fake, fake, 1, 8, 64, None, None, None) == -1
    assert L.lrs_masked_mse_cmask_f32(fake, fake, fake, 8, 0, 64, None, fake, None) == -1
    assert L.lrs_masked_mse_cmask_f32(fake, fake, fake, 8, 8, 0, None, fake, None) == -1
    for mc in (0, 2, 7, 9, -1):
        assert L.lrs_masked_mse_cmask_f32(fake, fake, fake, mc, 8, 64, None, fake, None) == -1, mc
    # an unbound net (no workspace) is refused as lrs_dipnet_train_steps refuses it
    from lrspnp.dip import DipNode, conv_node
    nodes = (DipNode * 1)(conv_node(0, 0, 8, 1, bn=0))
    h = ctypes.c_void_p()
    assert L.lrs_dipnet_create(nodes, 1, 8, 6, 6, None, ctypes.byref(h)) == 0
    try:
        assert L.lrs_dipnet_train_steps_cmask(h, fake, fake, fake, 8, f(0.1), f(0.9), f(0.999), f(1e-8), None, None,
                                              1, 0, None) == -1
    finally:
        L.lrs_dipnet_destroy(h)

"""Host: the reflected frame of the DIP prox (lrspnp.dip.frame_for, DipConfig.frame) and the argument
checks of its entry points -- nothing here touches a device.

The 1-Lipschitz U-Net maps H back to H only for H = 16 m - 12 (four stride-2 3x3 convs, two unpadded
2x2 up-convs): the smallest such size >= H is 16 ceil((H + 12) / 16) - 12.  By hand: 36 -> 36,
196 -> 196, 200 -> 212, 145 -> 148.
"""
import ctypes

import pytest

from lrspnp import _lib
from lrspnp.dip import DipConfig, DipProx, frame_for, lipschitz_unet_nodes, net_out_hw, skip_nodes, unet_size_ok


def unet_frame(H):
    return 16 * -(-(H + 12) // 16) - 12


def test_formula_by_hand():
    assert [unet_frame(h) for h in (36, 196, 200, 145)] == [36, 196, 212, 148]


@pytest.mark.parametrize("H", [36, 196, 200, 145, 40, 37, 16])
def test_frame_for_unet(H):
    nodes = lipschitz_unet_nodes(7, 7, 128)
    Hf = unet_frame(H)
    assert frame_for(nodes, H, H) == (Hf, Hf, (Hf - H) // 2, (Hf - H) // 2)
    assert unet_size_ok(Hf, Hf) and net_out_hw(nodes, Hf, Hf) == (Hf, Hf)
    assert not any(unet_size_ok(h, h) for h in range(H, Hf))     # the smallest


def test_frame_for_the_cases_of_the_gpu_tests():
    nodes = lipschitz_unet_nodes(7, 7, 128)
    assert frame_for(nodes, 40, 40) == (52, 52, 6, 6)            # even pads 6 / 6
    assert frame_for(nodes, 37, 45) == (52, 52, 7, 3)            # odd pads 7 / 8 and 3 / 4
    assert frame_for(nodes, 36, 36) == (36, 36, 0, 0)
    assert frame_for(nodes, 610, 340) == (612, 340, 1, 0)        # Pavia U: one axis framed
    assert frame_for(skip_nodes(7, 7), 37, 45) == (37, 45, 0, 0)  # the skip net crops: it reproduces every size


@pytest.mark.parametrize("hw", [(5, 40), (40, 5), (1, 36), (7, 7)])
def test_pad_reaching_the_dimension_is_refused(hw):
    """5 -> 20 needs pads 7 / 8 >= 5; 7 -> 20 needs 6 / 7 >= 7 (ReflectionPad2d wants pad < size)."""
    with pytest.raises(ValueError, match="reaches the dimension"):
        frame_for(lipschitz_unet_nodes(7, 7, 128), *hw)
    assert frame_for(lipschitz_unet_nodes(7, 7, 128), 8, 8) == (20, 20, 6, 6)   # 6 / 6 < 8 is taken


def test_frame_off_raises_as_before():
    """frame='off' at 40x40 stops where every size the net does not reproduce stopped: ValueError
    from DipProx.__init__, before any device work (creating the host object needs none)."""
    with pytest.raises(ValueError, match="needs sizes it reproduces"):
        DipProx(7, 40, 40, DipConfig(frame="off"))
    with pytest.raises(ValueError, match="'auto' or 'off'"):
        DipProx(7, 40, 40, DipConfig(frame="reflect"))
    assert DipConfig().frame == "auto"


def test_version_and_argument_checks():
    L = _lib.lib()
    assert L.lrs_version().startswith(b"lrspnp-hip 0.2.1")
    fake = ctypes.c_void_p(256)
    ok = (40, 40, 7, 6, 6, 52, 52)
    # (X, L, c, H, W, B, top, left, Hf, Wf, img, stream)
    assert L.lrs_unfolded_to_frame_f32(None, None, 1.0, *ok, fake, None) == -1
    assert L.lrs_unfolded_to_frame_f32(fake, None, 1.0, *ok, None, None) == -1
    assert L.lrs_frame_to_unfolded_f32(None, *ok, fake, None) == -1
    for bad in ((40, 40, 7, 13, 6, 52, 52),      # the image leaves the frame
                (40, 40, 7, -1, 6, 52, 52),
                (5, 40, 7, 7, 6, 20, 52),        # top pad 7 >= 5
                (5, 40, 7, 4, 6, 20, 52),        # bottom pad 11 >= 5
                (40, 40, 0, 6, 6, 52, 52)):
        assert L.lrs_unfolded_to_frame_f32(fake, None, 1.0, *bad, fake, None) == -1, bad
        assert L.lrs_frame_to_unfolded_f32(fake, *bad, fake, None) == -1, bad
    # (out, target, mask, mask_channels, C, P, n_mean, gout, loss_acc, stream): 0 < n_mean <= C P
    for n in (0, -3, 7 * 2704 + 1):
        assert L.lrs_masked_mse_framed_f32(fake, fake, fake, 1, 7, 2704, n, None, fake, None) == -1, n
    assert L.lrs_masked_mse_framed_f32(fake, fake, fake, 2, 7, 2704, 7 * 1600, None, fake, None) == -1


def test_set_frame_on_the_host_object():
    """lrs_dipnet_set_frame checks the frame against the net's output; the whole output is no frame."""
    from lrspnp.dip import DipNode
    L = _lib.lib()
    nodes = lipschitz_unet_nodes(7, 7, 128)
    arr = (DipNode * len(nodes))(*nodes)
    h = ctypes.c_void_p()
    opts = _lib.dip_opts()
    assert L.lrs_dipnet_create(arr, len(nodes), 7, 52, 52, ctypes.byref(opts), ctypes.byref(h)) == 0
    try:
        got = [ctypes.c_int() for _ in range(4)]
        assert L.lrs_dipnet_get_frame(h, *[ctypes.byref(g) for g in got]) == 0
        assert [g.value for g in got] == [0, 0, 52, 52]
        assert L.lrs_dipnet_set_frame(h, 6, 6, 40, 40) == 0
        assert L.lrs_dipnet_set_frame(h, 7, 3, 37, 45) == 0
        assert L.lrs_dipnet_get_frame(h, *[ctypes.byref(g) for g in got]) == 0
        assert [g.value for g in got] == [7, 3, 37, 45]
        assert L.lrs_dipnet_set_frame(h, 13, 6, 40, 40) == -1      # outside the output
        assert L.lrs_dipnet_set_frame(h, 24, 6, 5, 40) == -1       # pad >= the dimension
        assert [g.value for g in got] == [7, 3, 37, 45]
        assert L.lrs_dipnet_set_frame(h, 0, 0, 52, 52) == 0
    finally:
        L.lrs_dipnet_destroy(h)

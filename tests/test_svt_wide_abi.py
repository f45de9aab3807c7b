"""Host-side ABI of the wide-band SVT path (256 < B <= 512); no GPU needed."""
import ctypes

from lrspnp import _lib


def test_max_bands():
    assert _lib.lib().lrs_svt_max_bands() == 512
    from lrspnp import ops
    assert ops.svt_max_bands() == 512


def test_workspace_grows_with_the_band_count():
    L = _lib.lib()
    w256, w512 = L.lrs_svt_workspace(4000, 256), L.lrs_svt_workspace(4000, 512)
    assert w512 > w256 > 0
    # the rotation log of the Jacobi chain alone: kMaxSweeps (40) x 511 rounds x 256 pairs x (c, s) fp64
    assert w512 > 40 * 511 * 256 * 16
    # DESIGN.md §4 records this figure
    assert L.lrs_svt_workspace(40000, 512) == 130916864


# B: (lrs_svt_workspace(40000, B), lrs_svt_gram_offset(40000, B) bytes or None where it refuses), read
# from the library of commit 5d4508b, before the layout became a table of offsets.  Both sides of every
# shape-class boundary (198 | 199, 200 | 201, 208 | 209, 256 | 257) and the ends of the range.
LAYOUT_5D4508B = {
    7: (47739588, 47710464),
    45: (48572068, 47710464),
    198: (63335568, 47710464),
    199: (63647940, 47710464),
    200: (63650304, 47710464),
    201: (64013636, 47710464),
    208: (64993280, 47710464),
    209: (88917380, 71303424),
    224: (91334656, 71303424),
    256: (97440256, 71303424),
    257: (34449668, None),
    320: (51348992, None),
    512: (130916864, None),
}


def test_workspace_layout_is_the_one_callers_allocated_before():
    """Workspaces and Gram views (row-slab shards all-reduce G in place) are sized by the caller from
    these two calls: every offset and the total stay byte for byte what they were."""
    L = _lib.lib()
    for B, (total, goff) in LAYOUT_5D4508B.items():
        assert L.lrs_svt_workspace(40000, B) == total, B
        off, ld = ctypes.c_int64(-1), ctypes.c_int64(-1)
        rc = L.lrs_svt_gram_offset(40000, B, ctypes.byref(off), ctypes.byref(ld))
        if goff is None:
            assert rc == -2, B
        else:
            assert (rc, off.value, ld.value) == (0, goff, B + (B & 1)), B


def test_gram_offset_still_refuses_wide_cubes():
    """Row-slab sharding of wide cubes is out of scope: the wide path's eigen stage is the warm
    Jacobi chain, which lrs_svt_gram_offset's contract excludes."""
    L = _lib.lib()
    off, ld = ctypes.c_int64(), ctypes.c_int64()
    assert L.lrs_svt_gram_offset(4000, 300, ctypes.byref(off), ctypes.byref(ld)) == -2
    assert L.lrs_svt_gram_offset(4000, 512, ctypes.byref(off), ctypes.byref(ld)) == -2
    assert L.lrs_svt_gram_offset(4000, 256, ctypes.byref(off), ctypes.byref(ld)) == 0 and ld.value == 256


def test_refusals_come_before_any_device_work():
    """Above 512 bands, and LRS_SVT_MULTI_WG above 256: LRS_E_UNSUPPORTED; a short workspace:
    LRS_E_WORKSPACE.  The pointers are never dereferenced (the checks come first)."""
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)
    big = 1 << 40
    for B in (513, 514, 600):
        assert L.lrs_svt_gram_f32(fake, None, 1.0, 1000, B, 0, fake, big, None) == -2
        assert L.lrs_svt_finish_f32(fake, None, 1.0, 1000, B, 1.0, fake, None, 0, fake, big, None) == -2
        assert L.lrs_svt_f32(fake, None, 1.0, 1000, B, 1.0, fake, None, 0, fake, big, None) == -2
    for flags in (4, 5):
        assert L.lrs_svt_gram_f32(fake, None, 1.0, 1000, 300, flags, fake, big, None) == -2
        assert L.lrs_svt_finish_f32(fake, None, 1.0, 1000, 300, 1.0, fake, None, flags, fake, big, None) == -2
        assert L.lrs_svt_f32(fake, None, 1.0, 1000, 300, 1.0, fake, None, flags, fake, big, None) == -2
    need = L.lrs_svt_workspace(1000, 300)
    assert L.lrs_svt_gram_f32(fake, None, 1.0, 1000, 300, 0, fake, need - 1, None) == -3
    assert L.lrs_svt_finish_f32(fake, None, 1.0, 1000, 300, 1.0, fake, None, 0, fake, need - 1, None) == -3

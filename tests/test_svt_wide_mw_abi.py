"""Host-side ABI of LRS_SVT_WIDE_MW, the many-workgroup Householder reduction of the wide tridiagonal
chain (256 < B <= 512, with LRS_SVT_WIDE_TRI); no GPU needed."""
import ctypes
import os
import re

import pytest

from lrspnp import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# lrs_svt_workspace(40000, B): 257, 320 and 512 as tests/test_svt_wide_abi.py pins them; the others read
# from the library of the commit before this flag (the layout is that file's table of offsets)
WORKSPACE_40000 = {257: 34449668, 258: 34452752, 300: 45486912, 320: 51348992, 448: 100331008, 511: 130910724,
                   512: 130916864}


def test_flag_value():
    with open(os.path.join(REPO, "include", "lrspnp.h")) as fh:
        m = re.search(r"^#define\s+LRS_SVT_WIDE_MW\s+(\d+)\s*$", fh.read(), re.M)
    assert m and int(m.group(1)) == 16
    assert _lib.SVT_WIDE_MW == 16
    from lrspnp import ops
    assert ops.SVT_WIDE_MW == 16
    assert ops._svt_flags(False, "tri", wide_tri=True, wide_mw=True) == 24
    assert ops._svt_flags(True, "jacobi", wide_tri=True, wide_mw=True) == 27
    assert ops._svt_flags(True, "tri", wide_tri=True) == 9


def test_workspace_is_byte_for_byte_what_it_was():
    L = _lib.lib()
    for B, total in WORKSPACE_40000.items():
        assert L.lrs_svt_workspace(40000, B) == total, B


def test_gram_offset_still_refuses_wide_cubes():
    L = _lib.lib()
    off, ld = ctypes.c_int64(), ctypes.c_int64()
    assert L.lrs_svt_gram_offset(40000, 257, ctypes.byref(off), ctypes.byref(ld)) == -2
    assert L.lrs_svt_gram_offset(40000, 512, ctypes.byref(off), ctypes.byref(ld)) == -2


def test_refusals_come_before_any_device_work():
    """LRS_SVT_MULTI_WG above 256 bands stays LRS_E_UNSUPPORTED with the new bit set, as does B > 512; a
    short workspace is LRS_E_WORKSPACE.  The pointers are never dereferenced (the checks come first)."""
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)
    big = 1 << 40
    for flags in (16 | 8 | 4, 16 | 4, 16 | 8 | 4 | 1):
        assert L.lrs_svt_gram_f32(fake, None, 1.0, 1000, 300, flags, fake, big, None) == -2
        assert L.lrs_svt_finish_f32(fake, None, 1.0, 1000, 300, 1.0, fake, None, flags, fake, big, None) == -2
        assert L.lrs_svt_f32(fake, None, 1.0, 1000, 300, 1.0, fake, None, flags, fake, big, None) == -2
    assert L.lrs_svt_finish_f32(fake, None, 1.0, 1000, 513, 1.0, fake, None, 24, fake, big, None) == -2
    need = L.lrs_svt_workspace(1000, 300)
    assert L.lrs_svt_finish_f32(fake, None, 1.0, 1000, 300, 1.0, fake, None, 24, fake, need - 1, None) == -3


def test_solver_config_mode_strings():
    from lrspnp import LrsPnPConfig
    from lrspnp._lib import LrsError
    from lrspnp.solver import svt_wide_solver_flags
    assert LrsPnPConfig().svt_wide_solver == "jacobi"
    assert LrsPnPConfig(svt_wide_solver="tri-mw").svt_wide_solver == "tri-mw"
    assert svt_wide_solver_flags("jacobi") == (False, False)
    assert svt_wide_solver_flags("tri") == (True, False)
    assert svt_wide_solver_flags("tri-mw") == (True, True)
    with pytest.raises(LrsError, match="svt_wide_solver"):
        svt_wide_solver_flags("qr")

"""Host-side ABI of LRS_SVT_WIDE_TRI, the opt-in tridiagonal eigen chain of wide cubes (256 < B <= 512);
no GPU needed."""
import ctypes
import os
import re

from lrspnp import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_value():
    with open(os.path.join(REPO, "include", "lrspnp.h")) as fh:
        m = re.search(r"^#define\s+LRS_SVT_WIDE_TRI\s+(\d+)\s*$", fh.read(), re.M)
    assert m and int(m.group(1)) == 8
    assert _lib.SVT_WIDE_TRI == 8
    from lrspnp import ops
    assert ops._svt_flags(True, "tri", wide_tri=True) == 9
    assert ops._svt_flags(False, "jacobi", wide_tri=True) == 10


def test_refusals_come_before_any_device_work():
    """LRS_SVT_MULTI_WG above 256 bands stays LRS_E_UNSUPPORTED with the new bit set, as does B > 512; a
    short workspace is LRS_E_WORKSPACE.  The pointers are never dereferenced (the checks come first)."""
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)
    big = 1 << 40
    for flags in (8 | 4, 8 | 4 | 1):
        assert L.lrs_svt_gram_f32(fake, None, 1.0, 1000, 300, flags, fake, big, None) == -2
        assert L.lrs_svt_finish_f32(fake, None, 1.0, 1000, 300, 1.0, fake, None, flags, fake, big, None) == -2
        assert L.lrs_svt_f32(fake, None, 1.0, 1000, 300, 1.0, fake, None, flags, fake, big, None) == -2
    assert L.lrs_svt_gram_f32(fake, None, 1.0, 1000, 513, 8, fake, big, None) == -2
    assert L.lrs_svt_finish_f32(fake, None, 1.0, 1000, 513, 1.0, fake, None, 8, fake, big, None) == -2
    assert L.lrs_svt_f32(fake, None, 1.0, 1000, 513, 1.0, fake, None, 8, fake, big, None) == -2
    need = L.lrs_svt_workspace(1000, 300)
    assert L.lrs_svt_gram_f32(fake, None, 1.0, 1000, 300, 8, fake, need - 1, None) == -3
    assert L.lrs_svt_finish_f32(fake, None, 1.0, 1000, 300, 1.0, fake, None, 8, fake, need - 1, None) == -3
    assert L.lrs_svt_f32(fake, None, 1.0, 1000, 300, 1.0, fake, None, 8, fake, need - 1, None) == -3


def test_solver_config_mode_string():
    from lrspnp import LrsPnPConfig
    assert LrsPnPConfig().svt_wide_solver == "jacobi"

"""The spectral NLM prox on the cube through the layers that need no GPU: the header declares its entry points,
the library exports them, lrspnp._lib binds them, lrspnp.ops wraps them, the solver knows the mode, and every
refusal of lrs_nlmcube_f32 is decided on the host before anything is launched (the pointers are never read)."""
import ctypes
import os
import re

import pytest

from lrspnp import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3


def test_header_declares_and_library_exports():
    src = open(os.path.join(REPO, "include", "lrspnp.h")).read()
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r"\bsize_t\s+lrs_nlmcube_workspace\s*\(", src)
    assert re.search(r"\bint\s+lrs_nlmcube_f32\s*\(", src)
    assert "admm_utils.py:95-100" in src
    assert hasattr(L, "lrs_nlmcube_workspace") and hasattr(L, "lrs_nlmcube_f32")


def test_lib_binds_the_signatures():
    L = _lib.lib()
    c = ctypes
    f32, f64, i32, i64, vp, sz = c.c_float, c.c_double, c.c_int, c.c_int64, c.c_void_p, c.c_size_t
    assert L.lrs_nlmcube_workspace.argtypes == [i64, i64, i64, i32, i32] and L.lrs_nlmcube_workspace.restype == sz
    assert L.lrs_nlmcube_f32.argtypes == [vp, vp, f32, i64, i64, i64, i32, i32, f64, f64, vp, vp, sz, vp]
    assert L.lrs_nlmcube_f32.restype == i32
    from lrspnp import ops
    for n in ("nlmcube_workspace", "nlmcube"):
        assert n in ops.__all__ and callable(getattr(ops, n)), n


def test_workspace_size():
    L = _lib.lib()
    ws = L.lrs_nlmcube_workspace
    for bad in ((0, 5, 5), (5, 0, 5), (5, 5, 0), (-1, 5, 5), (5, -3, 5), (5, 5, -7)):
        assert ws(*bad, 7, 2) == 0, bad
    for big in ((1 << 11, 1 << 10, 1 << 10), (1 << 31, 1, 1), (1 << 40, 1 << 40, 1 << 40)):
        assert ws(*big, 7, 2) == 0, big
    for ps, pd in ((4, 2), (0, 2), (9, 2), (7, -1), (7, 6)):
        assert ws(9, 11, 4, ps, pd) == 0, (ps, pd)
    # never shrinks as a size, the patch or the window grows (a one-launch design may need none at all)
    base = (12, 10, 8)
    for ps, pd in ((1, 0), (3, 3), (7, 2), (7, 5)):
        for k in range(3):
            last = 0
            for v in range(1, 40):
                s = list(base)
                s[k] = v
                n = ws(*s, ps, pd)
                assert n >= last, (s, ps, pd, n, last)
                last = n
    assert ws(*base, 7, 5) >= ws(*base, 7, 2) >= ws(*base, 3, 2) >= ws(*base, 1, 0)


def test_nlmcube_refuses_on_the_host():
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)
    H, W, B = 9, 11, 4
    need = L.lrs_nlmcube_workspace(H, W, B, 7, 2)
    ok = dict(X=fake, L2=fake, c2=0.5, H=H, W=W, B=B, ps=7, pd=2, h=0.05, sigma=0.0, U=fake, ws=fake, wsb=need)

    def call(**kw):
        a = dict(ok, **kw)
        return L.lrs_nlmcube_f32(a["X"], a["L2"], a["c2"], a["H"], a["W"], a["B"], a["ps"], a["pd"], a["h"], a["sigma"],
                                 a["U"], a["ws"], a["wsb"], None)

    nan, inf = float("nan"), float("inf")
    for k in ("X", "U"):
        assert call(**{k: None}) == INVALID, k
    for k in ("H", "W", "B"):
        assert call(**{k: 0}) == INVALID and call(**{k: -2}) == INVALID, k
    for ps in (0, -1, -3, 2, 4, 6, 8):
        assert call(ps=ps) == INVALID, ps
    assert call(pd=-1) == INVALID
    for h in (0.0, -0.05, nan, inf, -inf):
        assert call(h=h) == INVALID, h
    for s in (-1e-3, nan, -inf):
        assert call(sigma=s) == INVALID, s
    # the workspace: NULL only when none is needed; too few bytes otherwise
    if need > 0:
        assert call(ws=None) == INVALID
        assert call(wsb=need - 1) == WORKSPACE and call(wsb=0) == WORKSPACE
    # a patch or a window beyond the kernel's, H W B >= 2^31, whatever the workspace
    big = (1 << 63) - 1
    assert call(ps=9, wsb=big) == UNSUPPORTED and call(ps=101, wsb=big) == UNSUPPORTED
    assert call(pd=6, wsb=big) == UNSUPPORTED and call(pd=1000, wsb=big) == UNSUPPORTED
    assert call(H=1 << 11, W=1 << 10, B=1 << 10, wsb=big) == UNSUPPORTED
    assert call(H=1 << 31, W=1, B=1, wsb=big) == UNSUPPORTED
    assert call(H=1 << 40, W=1 << 40, B=1 << 40, wsb=big) == UNSUPPORTED
    # an invalid argument wins over both
    assert call(H=1 << 31, ps=4) == INVALID and call(ps=9, h=0.0) == INVALID and call(pd=6, sigma=-1.0) == INVALID
    assert call(pd=6, U=None) == INVALID and call(wsb=0, h=nan) == INVALID and call(H=1 << 31, pd=-1) == INVALID


def test_solver_config_is_checked_on_the_host():
    """The mode and its config's ranges, before any device work (no GPU here: nothing else can have run)."""
    from lrspnp import LrsError, LrsPnP, LrsPnPConfig, NlmCubeConfig
    from lrspnp import solver
    assert "nlm" in solver._MODES["lowrank"] and "nlm" in LrsPnP._PARTS
    assert LrsPnPConfig().nlm is None
    c = NlmCubeConfig()
    assert (c.patch_size, c.patch_distance, c.h, c.sigma) == (7, 2, 0.05, 0.0)
    c.check()
    for bad in (dict(patch_size=4), dict(patch_size=9), dict(patch_size=0), dict(patch_distance=6),
                dict(patch_distance=-1), dict(h=0.0), dict(h=float("nan")), dict(h=float("inf")), dict(sigma=-0.1),
                dict(sigma=float("nan"))):
        with pytest.raises(LrsError):
            NlmCubeConfig(**bad).check()
        with pytest.raises(LrsError, match="NlmCubeConfig"):
            LrsPnP(None, None, None, LrsPnPConfig(lowrank="nlm", nlm=NlmCubeConfig(**bad)), image_shape=(4, 4))

"""The TV prox on the cube through the layers that need no GPU: the header declares its entry points, the
library exports them, lrspnp._lib binds them, lrspnp.ops wraps them, and every refusal of lrs_tvprox_f32 is
decided on the host before anything is launched (the pointers are never read)."""
import ctypes
import os
import re

from lrspnp import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3


def test_header_declares_and_library_exports():
    src = open(os.path.join(REPO, "include", "lrspnp.h")).read()
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r"\bsize_t\s+lrs_tvprox_workspace\s*\(", src)
    assert re.search(r"\bint\s+lrs_tvprox_f32\s*\(", src)
    assert re.search(r"#define\s+LRS_TVPROX_WARM\s+1\b", src)
    assert hasattr(L, "lrs_tvprox_workspace") and hasattr(L, "lrs_tvprox_f32")


def test_lib_binds_the_signatures():
    L = _lib.lib()
    c = ctypes
    f32, f64, i32, i64, vp, sz = c.c_float, c.c_double, c.c_int, c.c_int64, c.c_void_p, c.c_size_t
    assert L.lrs_tvprox_workspace.argtypes == [i64, i64, i64] and L.lrs_tvprox_workspace.restype == sz
    assert L.lrs_tvprox_f32.argtypes == [vp, vp, f32, i64, i64, i64, f32, f32, f32, f64, i32, i32, vp, vp, vp, sz, vp]
    assert L.lrs_tvprox_f32.restype == i32
    assert _lib.TVPROX_WARM == 1
    from lrspnp import ops
    for n in ("tvprox_workspace", "tvprox"):
        assert n in ops.__all__ and callable(getattr(ops, n)), n


def test_workspace_size():
    L = _lib.lib()
    ws = L.lrs_tvprox_workspace
    for bad in ((0, 5, 5), (5, 0, 5), (5, 5, 0), (-1, 5, 5), (5, -3, 5), (5, 5, -7)):
        assert ws(*bad) == 0, bad
    assert ws(1 << 11, 1 << 10, 1 << 10) == 0 and ws(1 << 31, 1, 1) == 0 and ws(1 << 40, 1 << 40, 1 << 40) == 0
    assert ws(1, 1, 1) > 0
    # u, five p and five q arrays of H W B floats at least
    assert ws(9, 11, 4) >= 11 * 4 * 9 * 11 * 4
    base = (12, 10, 8)
    for k in range(3):
        last = 0
        for v in range(1, 40):
            s = list(base)
            s[k] = v
            n = ws(*s)
            assert n > 0 and n >= last, (s, n, last)
            last = n
        assert last > ws(*base)


def test_tvprox_refuses_on_the_host():
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)
    H, W, B = 9, 11, 4
    need = L.lrs_tvprox_workspace(H, W, B)
    ok = dict(X=fake, L2=fake, c2=0.5, H=H, W=W, B=B, sp=0.05, bd=0.02, ss=0.03, tau=1.5, n=3, flags=0, U=fake,
              stats=None, ws=fake, wsb=need)

    def call(**kw):
        a = dict(ok, **kw)
        return L.lrs_tvprox_f32(a["X"], a["L2"], a["c2"], a["H"], a["W"], a["B"], a["sp"], a["bd"], a["ss"], a["tau"],
                                a["n"], a["flags"], a["U"], a["stats"], a["ws"], a["wsb"], None)

    for k in ("X", "U", "ws"):
        assert call(**{k: None}) == INVALID, k
    for k in ("H", "W", "B"):
        assert call(**{k: 0}) == INVALID and call(**{k: -2}) == INVALID, k
    for k in ("sp", "bd", "ss", "tau"):
        assert call(**{k: -1e-3}) == INVALID and call(**{k: float("nan")}) == INVALID, k
    assert call(n=-1) == INVALID
    assert call(flags=2) == INVALID and call(flags=3) == INVALID and call(flags=-1) == INVALID
    # too small a workspace, with and without the warm flag
    assert call(wsb=need - 1) == WORKSPACE and call(wsb=0) == WORKSPACE and call(wsb=need - 1, flags=1) == WORKSPACE
    # H W B >= 2^31, whatever the workspace
    big = (1 << 63) - 1
    assert call(H=1 << 11, W=1 << 10, B=1 << 10, wsb=big) == UNSUPPORTED
    assert call(H=1 << 31, W=1, B=1, wsb=big) == UNSUPPORTED
    assert call(H=1 << 40, W=1 << 40, B=1 << 40, wsb=big) == UNSUPPORTED
    # an invalid argument wins over both
    assert call(H=1 << 31, n=-1) == INVALID and call(wsb=0, tau=-1.0) == INVALID

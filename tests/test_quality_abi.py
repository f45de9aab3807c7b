"""The quality monitor through the layers that need no GPU: the header declares its entry points, the library
exports them, lrspnp._lib binds them, lrspnp.ops and lrspnp.metrics wrap them, LrsPnP has run(), and every
refusal of the two calls is decided on the host before anything is launched (the pointers are never read)."""
import ctypes
import os
import re

from lrspnp import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3


def test_header_declares_and_library_exports():
    src = open(os.path.join(REPO, "include", "lrspnp.h")).read()
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r"\bsize_t\s+lrs_cube_quality_workspace\s*\(", src)
    assert re.search(r"\bint\s+lrs_cube_quality_f32\s*\(", src)
    assert re.search(r"\bint\s+lrs_keep_best_f32\s*\(", src)
    assert src.index("Quality monitor") > src.index("Metrics (not timed)")
    for n in ("lrs_cube_quality_workspace", "lrs_cube_quality_f32", "lrs_keep_best_f32"):
        assert hasattr(L, n), n


def test_lib_binds_the_signatures():
    L = _lib.lib()
    c = ctypes
    i32, i64, vp, sz = c.c_int, c.c_int64, c.c_void_p, c.c_size_t
    assert L.lrs_cube_quality_workspace.argtypes == [i64, i64] and L.lrs_cube_quality_workspace.restype == sz
    assert L.lrs_cube_quality_f32.argtypes == [vp, vp, vp, i64, i64, vp, vp, vp, sz, vp]
    assert L.lrs_keep_best_f32.argtypes == [vp, i32, c.c_int32, vp, vp, i64, vp, vp]
    from lrspnp import LrsPnP, metrics, ops, solver
    for n in ("cube_quality_workspace", "cube_quality", "keep_best"):
        assert n in ops.__all__ and callable(getattr(ops, n)), n
    assert callable(metrics.quality) and callable(LrsPnP.run)
    assert solver.HISTORY_COLUMNS[:3] == ("mpsnr", "sam_deg", "rel_err") and len(solver.HISTORY_COLUMNS) == 6


def test_workspace_size():
    ws = _lib.lib().lrs_cube_quality_workspace
    for bad in ((0, 5), (5, 0), (-1, 5), (5, -3)):
        assert ws(*bad) == 0, bad
    for big in ((1 << 31, 1), (1, 1 << 31), (1 << 16, 1 << 15), (1 << 40, 1 << 40), ((1 << 31) // 3 + 1, 3)):
        assert ws(*big) == 0, big
    for ok in (((1 << 31) - 1, 1), (1, (1 << 31) - 1), ((1 << 31) // 3, 3), (1, 1)):
        assert ws(*ok) > 0, ok
    # a function of B alone below the limit (the slab count is fixed), and it grows with B
    assert ws(1, 198) == ws(38416, 198) == ws(1 << 20, 198)
    last = 0
    for B in (1, 2, 63, 64, 65, 198, 512, 513, 4000):
        assert ws(100, B) > last
        last = ws(100, B)


def test_calls_refuse_on_the_host():
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)
    P, B = 40, 6
    need = L.lrs_cube_quality_workspace(P, B)
    ok = dict(X=fake, C=fake, region=fake, P=P, B=B, q=fake, pb=fake, ws=fake, wsb=need)

    def call(**kw):
        a = dict(ok, **kw)
        return L.lrs_cube_quality_f32(a["X"], a["C"], a["region"], a["P"], a["B"], a["q"], a["pb"], a["ws"], a["wsb"],
                                      None)

    for k in ("X", "C", "q", "ws"):
        assert call(**{k: None}) == INVALID, k
    for k in ("P", "B"):
        assert call(**{k: 0}) == INVALID and call(**{k: -2}) == INVALID, k
    assert call(wsb=need - 1) == WORKSPACE and call(wsb=0) == WORKSPACE
    big = (1 << 63) - 1
    assert call(P=1 << 31, B=1, wsb=big) == UNSUPPORTED and call(P=1 << 16, B=1 << 15, wsb=big) == UNSUPPORTED
    assert call(P=1 << 40, B=1 << 40, wsb=big) == UNSUPPORTED
    assert call(P=1 << 31, X=None) == INVALID            # an invalid argument wins

    far = ctypes.c_void_p(1 << 20)

    def keep(score=fake, sign=1, src=fake, dst=far, n=16, best=fake):
        return L.lrs_keep_best_f32(score, sign, 3, src, dst, n, best, None)

    for k in ("score", "src", "dst", "best"):
        assert keep(**{k: None}) == INVALID, k
    for s in (0, 2, -2, 100):
        assert keep(sign=s) == INVALID, s
    assert keep(n=0) == INVALID and keep(n=-5) == INVALID
    assert keep(dst=fake) == INVALID                                          # the same buffer
    assert keep(dst=ctypes.c_void_p(4096 + 60)) == INVALID                    # the last float of src
    assert keep(src=ctypes.c_void_p(4096 + 60), dst=fake) == INVALID          # ... either way round


def test_run_refusals_need_no_device():
    """run()'s argument checks come before any device work: on a bare object nothing else can have run."""
    import pytest
    from lrspnp import LrsError, LrsPnP
    s = LrsPnP.__new__(LrsPnP)
    s.comm = None
    for kw in (dict(n_iter=0), dict(n_iter=3, keep_best="mpsnr"), dict(n_iter=3, clean=1, keep_best="best"),
               dict(n_iter=3, clean=1, region="rim")):
        with pytest.raises(LrsError):
            s.run(**kw)
    s.comm = object()
    with pytest.raises(LrsError, match="comm"):
        s.run(3)

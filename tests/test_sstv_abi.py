"""The TV term of the DIP output through the layers that need no GPU: the header declares its entry point,
the library exports it, lrspnp._lib binds it, lrspnp.ops wraps it, and the host-side argument checks refuse
before anything is launched."""
import ctypes
import os
import re

from lrspnp import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lrs_sstv_f32",)


def test_header_declares_and_library_exports():
    src = open(os.path.join(REPO, "include", "lrspnp.h")).read()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", src), n
        assert hasattr(L, n), n


def test_lib_binds_the_signatures():
    L = _lib.lib()
    f32, i32, vp = ctypes.c_float, ctypes.c_int, ctypes.c_void_p
    assert L.lrs_sstv_f32.argtypes == [vp] + [i32] * 7 + [f32] * 4 + [ctypes.c_int64, vp, vp, vp]
    from lrspnp import ops
    assert "sstv" in ops.__all__ and callable(ops.sstv)
    for n in NAMES:
        assert getattr(L, n).restype == i32


def test_sstv_refuses_on_the_host():
    """Every LRS_E_INVALID case of lrs_sstv_f32 is decided before a launch (the pointers are never read)."""
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)
    ok = dict(C=3, Hf=12, Wf=16, top=2, left=3, H=7, W=9, sp=0.05, bd=0.02, ss=0.03, eps=1e-3, n=3 * 7 * 9)

    def call(out=fake, **kw):
        a = dict(ok, **kw)
        return L.lrs_sstv_f32(out, a["C"], a["Hf"], a["Wf"], a["top"], a["left"], a["H"], a["W"], a["sp"], a["bd"],
                              a["ss"], a["eps"], a["n"], None, None, None)

    assert call(out=None) == -1
    for k in ("C", "Hf", "Wf", "H", "W"):
        assert call(**{k: 0}) == -1 and call(**{k: -1}) == -1, k
    assert call(top=-1) == -1 and call(left=-1) == -1
    assert call(top=6) == -1 and call(left=8) == -1 and call(H=13) == -1 and call(W=17) == -1   # does not fit
    for k in ("sp", "bd", "ss", "eps"):
        assert call(**{k: -1e-3}) == -1, k
    assert call(n=0) == -1 and call(n=-5) == -1
    # valid arguments with nothing to write, or with all weights 0: LRS_OK without a launch
    assert call() == 0
    assert call(sp=0.0, bd=0.0, ss=0.0) == 0

"""Every library symbol that Python names is one the built library exports (no GPU needed).

A tool that binds an entry point with ctypes keeps working only while the library exports it; the
prunes that remove diagnostics entry points are caught here instead of on the next GPU visit.
"""
import ctypes
import glob
import os
import re

from lrspnp import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = sorted(glob.glob(os.path.join(REPO, "tools", "*.py")) +
                 glob.glob(os.path.join(REPO, "lrs-pnp-dip_amd", "lrspnp", "*.py")))
# lrs_ names that are no functions: the struct types include/lrspnp.h declares (named in docstrings),
# a family written as a prefix ("lrs_dipnet_*": the match ends in "_"), and the mask's key in the data
# fixtures (data_img5.npz["lrs_mask"])
with open(os.path.join(REPO, "include", "lrspnp.h")) as _f:
    TYPES = set(re.findall(r"}\s*(lrs_[a-z0-9_]+)\s*;", _f.read()))
DATA_KEYS = {"lrs_mask"}


def _exported(L, name):
    try:
        getattr(L, name)
    except AttributeError:
        return False
    return True


def test_every_lrs_identifier_in_python_is_exported():
    assert len(SOURCES) > 10, SOURCES
    assert {"lrs_ista_opts", "lrs_dip_opts"} <= TYPES, TYPES
    L = ctypes.CDLL(_lib.LIB_PATH)
    missing = []
    for path in SOURCES:
        with open(path) as f:
            names = set(re.findall(r"\blrs_[a-z0-9_]+\b", f.read())) - TYPES - DATA_KEYS
            names = {n for n in names if not n.endswith("_")}
        missing += [(os.path.relpath(path, REPO), n) for n in sorted(names) if not _exported(L, n)]
    assert not missing, missing


def test_every_declared_signature_resolves():
    """_lib._declare() looks every key of its table up in the library: it raises on a missing one."""
    _lib._declare(ctypes.CDLL(_lib.LIB_PATH))

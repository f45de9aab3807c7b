"""The DIP engine's layout, pinned against values recorded from the commit before the per-node plan
(ca33aae): the workspace size, the parameter and running-statistics counts, every node's parameter
offsets and every tensor's shape, for the nets and sizes the product and the benchmark use and one
small odd size of each, with both precisions and both data-gradient forms of the upsampled convs.
The Deep Decoder's entries (DECODERS) were recorded the same way from c4be1a1.

lrs_dipnet_create needs no device, so this runs on the CPU.  The recorded table is
tests/golden/dipnet_layout.json; it was written by loading a build of ca33aae's library:

    LRSPNP_LIB=<liblrspnp_hip.so built from ca33aae> python tests/test_dipnet_layout.py --record
"""
import ctypes
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "lrs-pnp-dip_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from lrspnp import _lib  # noqa: E402
from lrspnp.dip import DipNode, deep_decoder_nodes, lipschitz_unet_nodes, skip_nodes  # noqa: E402

TABLE = os.path.join(HERE, "golden", "dipnet_layout.json")

# (net, bands, H, W): the 1-Lip U-Net at the benchmark's and the native size, the skip net at
# configs[3]'s size and at the literal 200 x 200 cube, and a small odd size of each
SIZES = [("unet", 198, 196, 196), ("unet", 128, 36, 36), ("unet", 7, 21, 19),
         ("skip", 224, 512, 512), ("skip", 198, 200, 200), ("skip", 5, 37, 35)]
CASES = [(net, C, H, W, prec, ud) for net, C, H, W in SIZES
         for prec in (_lib.DIP_F32, _lib.DIP_SPLIT_BF16) for ud in (0, 1)]

# The Deep Decoder (DECODE nodes; recorded from c4be1a1, the commit that added them, before they moved
# onto the node plan): (channels, c_out, h, w) of the input -- the measured 196^2 x 198 configuration, a
# 36^2 one, and a small, odd, non-square one; both precisions (it has no upsampled conv: ud = 0)
DECODERS = [((128, 128), 198, 49, 49), ((128, 128), 128, 9, 9), ((6, 4), 5, 7, 5)]
CASES += [("decoder", ch, cout, H, W, prec, 0) for ch, cout, H, W in DECODERS
          for prec in (_lib.DIP_F32, _lib.DIP_SPLIT_BF16)]


def case_id(c):
    if c[0] == "decoder":
        return "decoder%s-%d-%dx%d-p%d-ud%d" % (("-%d" * len(c[1])) % c[1], *c[2:])
    return "%s-%dx%dx%d-p%d-ud%d" % c


def layout(net, *case):
    if net == "decoder":
        channels, cout, H, W, prec, ud = case
        nodes, C = deep_decoder_nodes(channels[0], cout, channels), channels[0]
    else:
        C, H, W, prec, ud = case
        nodes = lipschitz_unet_nodes(C, C, 128) if net == "unet" else skip_nodes(C, C)
    L = _lib.lib()
    arr = (DipNode * len(nodes))(*nodes)
    h = ctypes.c_void_p()
    opts = _lib.dip_opts(prec, ud)
    rc = L.lrs_dipnet_create(arr, len(nodes), C, H, W, ctypes.byref(opts), ctypes.byref(h))
    assert rc == 0, rc
    try:
        out = {"workspace": int(L.lrs_dipnet_workspace(h)), "num_params": int(L.lrs_dipnet_num_params(h)),
               "num_bnstats": int(L.lrs_dipnet_num_bnstats(h)), "param_offsets": [], "node_shape": []}
        for i in range(len(nodes)):
            o = [ctypes.c_int64() for _ in range(4)]
            assert L.lrs_dipnet_param_offsets(h, i, *[ctypes.byref(x) for x in o]) == 0
            out["param_offsets"].append([x.value for x in o])
        for i in range(-1, len(nodes)):   # -1: the input tensor
            s = [ctypes.c_int() for _ in range(3)]
            assert L.lrs_dipnet_node_shape(h, i, *[ctypes.byref(x) for x in s]) == 0
            out["node_shape"].append([x.value for x in s])
        return out
    finally:
        L.lrs_dipnet_destroy(h)


@pytest.fixture(scope="module")
def table():
    with open(TABLE) as f:
        return json.load(f)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_layout_matches_recorded(table, case):
    want, got = table[case_id(case)], layout(*case)
    for key in ("workspace", "num_params", "num_bnstats", "param_offsets", "node_shape"):
        assert got[key] == want[key], key


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    with open(TABLE, "w") as f:
        json.dump({case_id(c): layout(*c) for c in CASES}, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")

"""One sha256 per output tensor of the DIP BatchNorm family, for bitwise A/B of two builds (LRSPNP_LIB).

    python tools/bn_forms_digest.py > new.txt
    LRSPNP_LIB=.../liblrspnp_hip_parent.so python tools/bn_forms_digest.py > parent.txt     # then diff

Primitive ABI: every case of tests/test_gpu_bn_forms.py (y, mean, invstd, running statistics, gz,
ggamma, gbeta, gbias).  Engine: three training steps from a fixed seed on the 36 x 36 x 7 and
66 x 66 x 7 U-Nets and the 36 x 36 x 128 skip net (output, parameters, gradients): the forms only the
engine launches (split-K finishing BatchNorm, accum, k_conv_bn_dir).
"""
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "lrs-pnp-dip_amd"))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import torch  # noqa: E402
from lrspnp import _lib  # noqa: E402
from lrspnp.dip import DipNet, lipschitz_unet_nodes, skip_nodes  # noqa: E402
from test_gpu_bn_forms import CASES, run_case  # noqa: E402


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


L = _lib.device_lib()
for C, HW, act in CASES:
    o, _ = run_case(L, C, HW, act)
    for k in ("y", "mean", "invstd", "run_mean", "run_var", "gz", "ggamma", "gbeta", "gbias"):
        print(f"bn C={C} P={HW} act={act} {k} {sha(o[k])}")

for name, nodes, bands, hw in (("unet36x7", lipschitz_unet_nodes(7, 7, 128), 7, 36),
                               ("unet66x7", lipschitz_unet_nodes(7, 7, 128), 7, 66),
                               ("skip36x128", skip_nodes(128, 128), 128, 36)):
    net = DipNet(nodes, bands, hw, hw)
    net.init_params(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand(bands, hw, hw, device="cuda", generator=g)
    Co, Ho, Wo = net.out_shape   # (a size that is no multiple of 4 comes out larger than it went in)
    t = torch.rand(Co, Ho, Wo, device="cuda", generator=g)
    m = (torch.rand(Ho, Wo, device="cuda", generator=g) > 0.2).float()
    net.train_steps(x, t, m, 3, use_graph=False)
    torch.cuda.synchronize()
    for k, v in (("output", net.output()), ("params", net.params), ("grads", net.grads), ("bnstats", net.bnstats)):
        print(f"net {name} {k} {sha(v)}")

"""sigma_max of every U-Net conv weight for several parameter seeds vs the fp64 SVD, in float32 ulp
(diagnostic; the suite asserts the same for three seeds: tests/test_gpu_sigma.py, family E)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in ("../lrs-pnp-dip_amd", "../tests"):
    sys.path.insert(0, os.path.join(HERE, p))
import torch  # noqa: E402
from lrspnp.dip import sigma_max  # noqa: E402
import sn_emu as E  # noqa: E402

for seed in list(range(20)) + [31, 1234]:
    mats = E.family_e((seed,))
    sig, _ = sigma_max([torch.from_numpy(m).cuda() for m in mats.values()])
    ulps = {k: E.ulp_err(s, E.sigma_ref(m)[0]) for (k, m), s in zip(mats.items(), sig.cpu().numpy())}
    print(f"seed {seed}: worst {max(ulps.values(), key=abs):+.2f} ulp;",
          {k: u for k, u in ulps.items() if abs(u) > 1.0}, flush=True)

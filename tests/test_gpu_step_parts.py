"""LrsPnP.step() against its public parts run one after another on the current stream: the low-rank method,
sparse_coding(), admm().  Every kernel is fixed-order, so two outer iterations of either leave the same bits in
X, L1, L2, U and Phi, in every low-rank mode and on every SVT chain the solver can pick.

The DIP row has the sizes of test_gpu_decoder.py::test_solver_runs_the_decoder (a 36 x 36 x 8 cube, decoder
channels (16, 16), so a 16 x 9 x 9 net input; bb = 8; 3 fixed steps)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STATE = ("X", "L1", "L2", "U", "phi")


def _problem(H, W, B):
    from lrspnp.data import mask_matrix, synthetic_cube, synthetic_dictionary, unfold
    obs, _, mask = synthetic_cube(H, W, B, seed=1)
    return unfold(obs), mask_matrix(mask, B), synthetic_dictionary(64, 64, 0)


def _decoder_cfg():
    from lrspnp import LrsPnPConfig
    from lrspnp.dip import DipConfig
    dip = DipConfig(net="decoder", decoder_channels=(16, 16), learning_rate=0.01, num_iter=3, early_stop=False)
    return LrsPnPConfig.dip_decoder(bb=8, sliding=8, Nit=10, variant="spec2", dip_seed=9, dip=dip)


def _svt(**kw):
    from lrspnp import LrsPnPConfig
    return LrsPnPConfig(bb=8, sliding=8, Nit=10, variant="spec2", **kw)


# id: (H = W, B, the config, the low-rank part)
MODES = {
    "svt": (24, 20, lambda: _svt(), lambda s: s.low_rank()),
    "svt-jacobi": (24, 20, lambda: _svt(svt_method="jacobi"), lambda s: s.low_rank()),
    "svt-wide": (24, 257, lambda: _svt(), lambda s: s.low_rank()),
    "svt-wide-tri": (24, 257, lambda: _svt(svt_wide_solver="tri"), lambda s: s.low_rank()),
    "svt-wide-tri-mw": (24, 257, lambda: _svt(svt_wide_solver="tri-mw"), lambda s: s.low_rank()),
    "tv": (24, 20, lambda: _svt(lowrank="tv"), lambda s: s.low_rank_tv()),
    "dip-decoder": (36, 8, _decoder_cfg, lambda s: s.low_rank_dip(torch.cuda.current_stream())),
}


@pytest.mark.parametrize("mode", list(MODES))
def test_step_equals_its_parts(mode):
    from lrspnp import LrsPnP
    hw, B, cfg, low_rank = MODES[mode]
    Y, M, D = _problem(hw, hw, B)
    whole, parts = (LrsPnP(Y, M, D, cfg(), image_shape=(hw, hw)) for _ in range(2))
    for _ in range(2):
        whole.step()
        low_rank(parts)
        parts.sparse_coding()
        parts.admm()
    torch.cuda.synchronize()
    assert whole.iteration == parts.iteration == 2
    for name in STATE:
        a, b = getattr(whole, name), getattr(parts, name)
        assert bool(torch.isfinite(a).all()), (mode, name)
        d = float((a - b).abs().max())
        print(f"{mode} {name}: max |step - parts| = {d:.3e}")
        assert torch.equal(a, b), (mode, name, d)
    assert float(np.abs(whole.X.cpu().numpy() - Y).max()) > 0   # the iterations moved X

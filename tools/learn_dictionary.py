#!/usr/bin/env python3
"""Learn the sparsifying dictionary of LRS-PnP from an observed cube (lrspnp.learn_dictionary).

    tools/learn_dictionary.py --cube noisy.mat --mask mask.mat --out trained_dictionary

reads the cube and the pixel mask through lrspnp.matio (.mat v5, converted v7.3, or .npz), trains on
the MI355X and writes <out>.npz (Dictionary, history) and <out>.mat, a MAT v5 file whose variable
`Dictionary` is what main_LRS_PnP.py:159-160 loads.

Cube orientation: a 3-D (B, H, W) array is taken as is; a 4-D array is taken as the h5py orientation
of the reference's v7.3 files (matio.cube_from_h5); --hwb marks a 3-D (H, W, B) array (a MATLAB v5
cube).  The mask is any array that squeezes to (H, W); it is applied to every band
(lrspnp.data.mask_matrix, main_LRS_PnP.py:188-192).
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lrs-pnp-dip_amd"))

from lrspnp import matio  # noqa: E402
from lrspnp.data import mask_matrix, unfold  # noqa: E402


def pick(d: dict, key, what: str) -> np.ndarray:
    if key is None:
        if len(d) != 1:
            raise SystemExit(f"{what}: variables {sorted(d)}; choose one with --{what}-key")
        key = next(iter(d))
    if key not in d:
        raise SystemExit(f"{what}: no variable {key!r} (has {sorted(d)})")
    return np.asarray(d[key])


def load_cube(path: str, key, hwb: bool) -> np.ndarray:
    a = pick(matio.load_mat(path), key, "cube")
    if a.ndim == 4:
        return matio.cube_from_h5(a)
    if a.ndim != 3:
        raise SystemExit(f"cube: expected a 3-D or 4-D array, got shape {a.shape}")
    a = a.astype(np.float32)
    return np.ascontiguousarray(a.transpose(2, 0, 1)) if hwb else a


def load_mask(path: str, key, shape) -> np.ndarray:
    m = np.squeeze(pick(matio.load_mat(path), key, "mask")).astype(np.float32)
    if m.shape != tuple(shape):
        raise SystemExit(f"mask: shape {m.shape} does not match the cube's {tuple(shape)}")
    return (m != 0).astype(np.float32)


def save(out: str, D: np.ndarray, history: np.ndarray):
    np.savez(out + ".npz", Dictionary=D, history=history)
    matio.save_mat5(out + ".mat", {"Dictionary": D})
    return out + ".npz", out + ".mat"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cube", required=True)
    ap.add_argument("--cube-key")
    ap.add_argument("--hwb", action="store_true", help="a 3-D cube is (H, W, B), not (B, H, W)")
    ap.add_argument("--mask", required=True)
    ap.add_argument("--mask-key")
    ap.add_argument("--out", required=True, help="output stem: <out>.npz and <out>.mat")
    ap.add_argument("--K", type=int, default=256)
    ap.add_argument("--bb", type=int, default=36)
    ap.add_argument("--train-sliding", type=int, default=None)
    ap.add_argument("--max-blocks", type=int, default=65536)
    ap.add_argument("--lambda-ista", type=float, default=0.1)
    ap.add_argument("--Nit", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--n-inner", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-normalise", action="store_true")
    a = ap.parse_args(argv)

    cube = load_cube(a.cube, a.cube_key, a.hwb)
    B, H, W = cube.shape
    mask = load_mask(a.mask, a.mask_key, (H, W))
    M = mask_matrix(mask, B)
    Y = unfold(cube) * M

    from lrspnp import DictLearnConfig, learn_dictionary
    cfg = DictLearnConfig(K=a.K, bb=a.bb, train_sliding=a.train_sliding, max_blocks=a.max_blocks,
                          lambda_ista=a.lambda_ista, Nit=a.Nit, rounds=a.rounds, n_inner=a.n_inner,
                          normalise=not a.no_normalise, seed=a.seed)
    D, history = learn_dictionary(Y, M, cfg)
    npz, mat = save(a.out, D.cpu().numpy(), history)
    print(f"{npz} {mat}: Dictionary {tuple(D.shape)}, objective {history[0, 0]:.6g} -> {history[-1, -1]:.6g} "
          f"over {a.rounds} rounds")


if __name__ == "__main__":
    main()

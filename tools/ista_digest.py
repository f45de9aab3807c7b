"""One sha256 per output tensor of the row-split and per-pattern ISTA kernels, for bitwise A/B of two builds.

    python tools/ista_digest.py > new.txt
    LRSPNP_LIB=.../liblrspnp_hip_parent.so python tools/ista_digest.py > parent.txt     # then diff

ops.ista and ops.ista_pat directly (not the solver), on seeded inputs, phi and coefs of every case:
row-split (k_ista_rs): bb 4, 5, 6, 8 (1 to 4 row tiles) x K 64, 100, 128, 200, 256, 512 x the three
proxes x accel off / fista, 40 blocks (two full column tiles and one of 8), Nit 5; where the resident
kernels serve (n_pad <= 64, K = 256, accel off, not the MATLAB prox) bb = 9 instead, once per prox with 40
blocks and with enough column tiles for the 3- and 2-wave forms.  One case on a single persistent
workgroup, and a warm-started continuation per accel.
per-pattern (k_ista_pat): bb 8 and 6 x K 64, 128, 200, 256, 512 x the proxes x accel, three patterns of
17, 16 and 7 blocks (a full tile, a 1-block tile, a ragged tile); 13 tiles unbounded (the XCD order with
a remainder) and on two workgroups; a warm-started continuation.
"""
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "lrs-pnp-dip_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from lrspnp import ops  # noqa: E402

PROXES = (("nlm", ops.PROX_NLM), ("soft", ops.PROX_SOFT), ("matlab", ops.PROX_NLM_MATLAB))
NIT = 5


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def inputs(bb, K, nb, seed, pats=None):
    """D (n, K) with unit columns, blocks Yb / obs padded to n_pad, alpha above ||D||_2^2, thr per block.
    pats (npat, n) u8 and the blocks' pattern indices when the masks are shared."""
    rng = np.random.default_rng(seed)
    n = bb * bb
    n_pad = -(-n // 16) * 16
    D = rng.standard_normal((n, K)).astype(np.float32)
    D /= np.linalg.norm(D, axis=0, keepdims=True)
    if pats is None:
        obs = (rng.random((nb, n)) > 0.2).astype(np.uint8)
    else:
        obs = pats[0][pats[1]]
    Yb = (rng.standard_normal((nb, n)) * 0.3).astype(np.float32) * obs
    alpha = (np.linalg.norm(D.astype(np.float64), 2) ** 2 * (1.0 + 0.2 * rng.random(nb))).astype(np.float32)
    thr = 0.02 * (1.0 + rng.random(nb))
    pad = lambda a: np.pad(a, ((0, 0), (0, n_pad - n)))
    return n, D, pad(Yb), pad(obs), alpha, thr, pad


def show(tag, phi, coefs):
    torch.cuda.synchronize()
    print(f"{tag} phi {sha(phi)}")
    print(f"{tag} coefs {sha(coefs)}")


# ---- row-split ------------------------------------------------------------------------------------
def resident(bb, K, prox, accel):
    """lrs_ista_f32 runs k_ista_res / k_ista_b3 / k_ista_ln2 there, not the row-split kernel."""
    return bb * bb <= 64 and K == 256 and accel == "off" and prox != ops.PROX_NLM_MATLAB


def rs_case(bb, K, pname, prox, accel, nb=40, **kw):
    n, D, Yb, obs, alpha, thr, _ = inputs(bb, K, nb, 1000 * bb + K)
    a = dict(Yb=d(Yb), obs=d(obs), D=d(D), n=n, alpha=d(alpha), thr=d(thr), prox=prox, accel=accel)
    tag = f"rs bb={bb} K={K} {pname} accel={accel}" + "".join(f" {k}={v}" for k, v in kw.items())
    warm = kw.pop("warm", False)
    phi, coefs = ops.ista(**a, Nit=NIT, want_coefs=True, **kw)
    if warm:   # continue from the first call's coefficients
        show(tag + " first", phi, coefs)
        phi, coefs = ops.ista(**a, Nit=NIT, coefs=coefs, want_coefs=True, warm_start=True)
    show(tag, phi, coefs)


for bb in (4, 5, 6, 8):
    for K in (64, 100, 128, 200, 256, 512):
        for pname, prox in PROXES:
            for accel in ("off", "fista"):
                if not resident(bb, K, prox, accel):
                    rs_case(bb, K, pname, prox, accel)
# K = 256, accel off, skimage / soft prox: the row-split kernel serves from n_pad = 80 up, so bb = 9 (6 row
# tiles).  Few column tiles take 4 waves; on 256 CUs the wave picker's makespan takes 3 waves at 1365 column
# tiles and 2 at 2048.  (The 1-wave form has one row tile, which is resident here: it runs the MATLAB prox only.)
for pname, prox in PROXES[:2]:
    for nb in (40, 16 * 1365, 16 * 2048):
        rs_case(9, 256, pname, prox, "off", nb=nb)
rs_case(6, 128, "nlm", ops.PROX_NLM, "off", nb=70, max_workgroups=1)
for accel in ("off", "fista"):
    rs_case(6, 200, "nlm", ops.PROX_NLM, accel, warm=True)


# ---- per-pattern ----------------------------------------------------------------------------------
def pat_case(bb, K, pname, prox, accel, counts=(17, 16, 7), **kw):
    n = bb * bb
    rng = np.random.default_rng(77 * bb + K)
    pats = (rng.random((len(counts), n)) > 0.2).astype(np.uint8)
    pat = rng.permutation(np.repeat(np.arange(len(counts)), counts)).astype(np.int32)
    n, D, Yb, _, alpha, thr, pad = inputs(bb, K, pat.size, 2000 * bb + K, (pats, pat))
    plan, nt = ops.ista_pat_plan(pat, len(counts))
    obs_pat = d(pad(pats))
    ws = ops.ista_pat_prepare(d(D), obs_pat, n)
    a = dict(Yb=d(Yb), obs_pat=obs_pat, plan=d(plan), ntiles=nt, K=K, n=n, alpha=d(alpha), thr=d(thr), ws=ws,
             prox=prox, accel=accel)
    tag = f"pat bb={bb} K={K} {pname} accel={accel} tiles={nt}" + "".join(f" {k}={v}" for k, v in kw.items())
    warm = kw.pop("warm", False)
    phi, coefs = ops.ista_pat(**a, Nit=NIT, want_coefs=True, **kw)
    if warm:
        show(tag + " first", phi, coefs)
        phi, coefs = ops.ista_pat(**a, Nit=NIT, coefs=coefs, want_coefs=True, warm_start=True)
    show(tag, phi, coefs)


for bb in (8, 6):
    for K in (64, 128, 200, 256, 512):
        for pname, prox in PROXES:
            for accel in ("off", "fista"):
                pat_case(bb, K, pname, prox, accel)
MANY = (70, 65, 40)   # 5 + 5 + 3 = 13 tiles: 13 = 8 + 5, the XCD order with a remainder
pat_case(6, 128, "nlm", ops.PROX_NLM, "off", counts=MANY)
pat_case(6, 128, "nlm", ops.PROX_NLM, "off", counts=MANY, max_workgroups=2)
pat_case(8, 200, "nlm", ops.PROX_NLM, "fista", warm=True)

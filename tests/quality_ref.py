"""fp64 numpy restatement of the quality monitor's definitions (include/lrspnp.h, "Quality monitor")
and of the keep-best rule.  Written from the definitions alone: nothing here is taken from the kernel."""
import numpy as np


def cube_quality(X, C, region=None):
    """X, C: (P, B) float32; region: None or (P, B), 1 = counted.  Returns q (4 doubles: MPSNR, SAM in degrees,
    relative error, pixels counted for SAM), psnr_bands (B doubles) and, for the tests' own bounds, sse_b, n_b and
    the counted pixels' angles in radians."""
    x, c = np.asarray(X, np.float32).astype(np.float64), np.asarray(C, np.float32).astype(np.float64)
    P, B = x.shape
    r = np.ones((P, B)) if region is None else (np.asarray(region) == 1).astype(np.float64)
    n_b = r.sum(0)
    sse_b = (r * (x - c) ** 2).sum(0)
    psnr = np.full(B, np.nan)
    for b in range(B):
        if n_b[b] > 0:
            mse = sse_b[b] / n_b[b]
            psnr[b] = 100.0 if mse < 1e-10 else 10.0 * np.log10(255.0 / np.sqrt(mse))
    q = np.full(4, np.nan)
    if (n_b > 0).any():
        q[0] = psnr[n_b > 0].mean()
    den = np.sqrt((x * x).sum(1)) * np.sqrt((c * c).sum(1))
    counted = (r.sum(1) > 0) & (den > 0)
    cos = np.clip((x * c).sum(1)[counted] / den[counted], -1.0, 1.0)
    angles = np.arccos(cos)
    q[3] = counted.sum()
    if q[3] > 0:
        q[1] = np.degrees(angles.mean())
    c2 = (r * c * c).sum()
    if c2 > 0:
        q[2] = np.sqrt(sse_b.sum()) / np.sqrt(c2)
    return dict(q=q, psnr_bands=psnr, sse_b=sse_b, n_b=n_b, angles=angles)


def better(score, best, sign):
    """The keep-best rule: strictly better in the direction of sign; NaN never wins, a NaN best always loses."""
    if np.isnan(score):
        return False
    return bool(np.isnan(best) or sign * score > sign * best)


def keep_best(scores, sign, snapshots):
    """Run the rule over a sequence from best = (NaN, NaN) and dst = None.  Returns, after every call, the pair
    (best score, best iteration) and the index of the snapshot dst holds (None: never written)."""
    best, it, held, out = np.nan, np.nan, None, []
    for t, s in enumerate(scores):
        if better(s, best, sign):
            best, it, held = s, float(t), t
        out.append((best, it, None if held is None else snapshots[held]))
    return out

"""CPU fp64 model of the spectral-norm chain (csrc/dip_sn.h: k_sn_gram, k_sn_gram_reduce, k_sn_sigma,
k_sn_apply) and the operand sets of its tests.

Imported by tests/test_sn_emu.py (CPU: the model against the fp64 SVD, and the proof that the cases have
teeth) and tests/test_gpu_sigma.py (the kernels against the fp64 SVD on the same matrices).

The model follows the kernel statement by statement: the fp64 Gram of the float32 values on the smaller
side, summed per inner split (16 splits of round_up(ceil(inner / 16), 32)) and then over the splits in
order; Lanczos on the unnormalised residual from the start vector 1 + 0.5 sin(0.7 i + 0.3) with the
b > 1e-14 |a_last| break; checks at k + 1 >= 24, (k + 1) % 4 == 0 with sn_grid / sn_round / sn_multisect
and the have / converged / re-bracket logic; the final 257x narrowing and lmax = (lo + hi) / 2.  What it
does not reproduce is the order of the fp64 sums inside a matvec or an MFMA (relative 1e-16, nine decades
below a float32 ulp) and whether the compiler contracts sn_grid to one fma.

The Sturm count is the kernel's: the fast path (terms unperturbed, rescaled by a power of two every 8
terms, an exact zero only recorded) and, for the lanes that met a zero, the checked path (a zero term is
perturbed to -p 2^-600, rescaled every 4 terms).  Both are evaluated for 256 abscissae at once.

Degraded variants (keyword switches of sigma_model, VARIANTS) are the teeth of the cases: first_bracket,
first_check, gram_f32, drop_tail, no_zero_convention, coarse_tol, and prescale=False (the chain as it was
before sn_scale).
"""
import functools
import math

import numpy as np

MAX_DIM = 128
SPLIT = 16


# ---- the Gram ------------------------------------------------------------------------------------

def gram(W, gram_f32=False, drop_tail=False):
    """G = W W^T (rows <= cols) or W^T W of a float32 matrix, summed as k_sn_gram + k_sn_gram_reduce.
    gram_f32: products and sums in float32.  drop_tail: the last non-empty split loses the part of its
    range that does not fill a 32-chunk (a wrong k < ke guard)."""
    W = np.asarray(W)
    assert W.dtype == np.float32 and W.ndim == 2
    A = W if W.shape[0] <= W.shape[1] else W.T
    m, inner = A.shape
    assert m <= MAX_DIM
    per = -(-(-(-inner // SPLIT)) // 32) * 32
    dt = np.float32 if gram_f32 else np.float64
    A = A.astype(dt)
    G = np.zeros((m, m), dt)
    for z in range(SPLIT):
        kb, ke = z * per, min(inner, (z + 1) * per)
        if kb >= ke:
            continue
        if drop_tail and ke == inner:
            ke = kb + (ke - kb) // 32 * 32
        if gram_f32:
            P = np.zeros((m, m), np.float32)
            for k in range(kb, ke):                         # rank-1 updates in k order, every sum rounded
                P = P + np.outer(A[:, k], A[:, k])
        else:
            P = A[:, kb:ke] @ A[:, kb:ke].T
        G = G + P
    return G.astype(np.float64)


# ---- Sturm counts --------------------------------------------------------------------------------

def _rescale(p, pm):
    with np.errstate(invalid="ignore"):
        _, e = np.frexp(np.where(np.abs(p) > np.abs(pm), p, pm))
    return np.ldexp(p, -e), np.ldexp(pm, -e)


def _sturm_checked(a, b2, n, x, s0):
    pm = np.full_like(x, s0)
    p = (a[0] - x) * s0
    p = np.where(p != 0.0, p, -s0 * 2.0 ** -600)
    changes = (p < 0.0).astype(np.int64)

    def term(i, p, pm, changes):
        pn = (a[i] - x) * p - b2[i] * pm
        pn = np.where(pn != 0.0, pn, -p * 2.0 ** -600)
        return pn, p, changes + (np.signbit(pn) != np.signbit(p))
    i = 1
    while i + 4 <= n:
        for j in range(4):
            p, pm, changes = term(i + j, p, pm, changes)
        p, pm = _rescale(p, pm)
        i += 4
    while i < n:
        p, pm, changes = term(i, p, pm, changes)
        i += 1
    return n - changes


def sturm_gt(a, b2, n, x, s0=1.0, stats=None, no_zero_convention=False):
    """Eigenvalues of T_n (diagonal a, squared off-diagonals b2[i] = beta_{i-1}^2) above each x: sturm_gt,
    the sequence started from p_0 = s0, p_1 = (a_0 - x) s0.  no_zero_convention: an exact zero is neither
    perturbed nor re-evaluated; it takes its predecessor's sign."""
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        pm = np.full_like(x, s0)
        p = (a[0] - x) * s0
        zero = p == 0.0
        changes = (p < 0.0).astype(np.int64)

        def term(i, p, pm, changes, zero):
            pn = (a[i] - x) * p - b2[i] * pm
            if no_zero_convention:
                pn = np.where(pn == 0.0, np.copysign(0.0, p), pn)
            return pn, p, changes + (np.signbit(pn) != np.signbit(p)), zero | (pn == 0.0)
        i = 1
        while i + 8 <= n:
            for j in range(8):
                p, pm, changes, zero = term(i + j, p, pm, changes, zero)
            if stats is not None and not (np.isfinite(p).all() and np.isfinite(pm).all()):
                stats["nonfinite"] += 1
            p, pm = _rescale(p, pm)
            i += 8
        while i < n:
            p, pm, changes, zero = term(i, p, pm, changes, zero)
            i += 1
        if stats is not None and not np.isfinite(p).all():
            stats["nonfinite"] += 1
        count = n - changes
        if zero.any() and not no_zero_convention:
            if stats is not None:
                stats["checked"] += int(zero.sum())
            count = np.where(zero, _sturm_checked(a, b2, n, x, s0), count)
    return count


# ---- multisection --------------------------------------------------------------------------------

_T1 = np.arange(1, 257, dtype=np.float64)


def sn_grid(base, step, t):
    return base + step * float(t + 1)


def sn_scale(top, prescale=True):
    """2^-e with top = f 2^e, 0.5 <= f < 1 (1 for a top that is not positive and finite): sn_scale."""
    if not prescale or not (0.0 < top < 1e300):
        return 1.0
    return math.ldexp(1.0, -math.frexp(top)[1])


def sn_round(a, b2, n, base, step, stats, prescale=True, **kw):
    """Largest t in 0..255 with an eigenvalue above base + step (t + 1), or -1."""
    stats["rounds"] += 1
    s0 = sn_scale(sn_grid(base, step, 255), prescale)
    hit = np.nonzero(sturm_gt(a, b2, n, base + step * _T1, s0, stats, **kw) >= 1)[0]
    return int(hit[-1]) if hit.size else -1


def sn_multisect(a, b2, n, lo, hi, tol, stats, **kw):
    it = 0
    while it < 12 and hi - lo > tol * hi:
        step = (hi - lo) * (1.0 / 257.0)
        bt = sn_round(a, b2, n, lo, step, stats, **kw)
        nlo = sn_grid(lo, step, bt) if bt >= 0 else lo
        nhi = sn_grid(lo, step, bt + 1) if bt < 255 else hi
        lo, hi = nlo, max(nlo, nhi)
        it += 1
    return lo, hi


# ---- the chain -----------------------------------------------------------------------------------

def start_vector(m):
    return 1.0 + 0.5 * np.sin(0.7 * np.arange(m, dtype=np.float64) + 0.3)


def new_stats():
    return {"steps": 0, "rounds": 0, "checks": 0, "checked": 0, "nonfinite": 0, "rebracket": 0, "moved": 0,
            "break": 0, "converged": 0, "exhausted": 0}


def lambda_max(G, stats=None, first_bracket=False, first_check=24, no_zero_convention=False, coarse_tol=False,
               prescale=True, start=None):
    """k_sn_sigma's top eigenvalue of the m x m Gram.  stats (new_stats()) receives the step and branch
    counters.  start: another start vector (the family-F experiments)."""
    stats = new_stats() if stats is None else stats
    kw = {"no_zero_convention": no_zero_convention, "prescale": prescale}
    m = G.shape[0]
    a = np.zeros(MAX_DIM)
    b2 = np.zeros(MAX_DIM)
    r = start_vector(m) if start is None else np.asarray(start, np.float64).copy()
    qprev = np.zeros(m)
    gmax, gmin, a_last, b_last = -1e300, 1e300, 0.0, 0.0
    blo = bhi = 0.0
    have = converged = False
    tol_bracket, tol_final = (1e-6, 1e-6) if coarse_tol else (5e-10, 1e-12)
    k = 0
    with np.errstate(all="ignore"):
        while k < m:
            u = G @ r
            s_rr, s_ru = float(r @ r), float(r @ u)
            b = math.sqrt(s_rr) if s_rr >= 0.0 else float("nan")
            if k > 0 and not (b > 1e-14 * abs(a_last)):
                stats["break"] += 1
                break
            ib = 1.0 / b
            al = s_ru * ib * ib
            a[k], b2[k] = al, s_rr
            if k > 0:
                rad = b_last + b
                gmax = max(gmax, a_last + rad)
                gmin = min(gmin, a_last - rad)
            a_last = al
            b_last = b if k > 0 else 0.0
            qk = r * ib
            r = u * ib - al * qk - (b if k > 0 else 0.0) * qprev
            qprev = qk
            if k + 1 == m:
                k += 1
                stats["exhausted"] += 1
                break
            if k + 1 >= first_check and (k + 1) % 4 == 0:
                stats["checks"] += 1
                n = k + 1
                hi = max(gmax, a_last + b_last)
                need = True
                if have:
                    w = bhi - blo
                    bt = sn_round(a, b2, n, blo, w, stats, **kw)
                    if bt < 0:
                        converged, need = True, False
                    elif bt < 255:
                        b0 = blo
                        blo, bhi = sn_grid(b0, w, bt), sn_grid(b0, w, bt + 1)
                        need = False
                        stats["moved"] += 1
                    else:
                        lo = sn_grid(blo, w, 255)
                        stats["rebracket"] += 1
                else:
                    lo = max(0.0, min(gmin, a_last - b_last))
                if need:
                    lo, hi = sn_multisect(a, b2, n, lo, hi, tol_bracket, stats, **kw)
                    blo, bhi, have = lo, hi, True
                    if first_bracket:
                        converged = True
                if converged:
                    k += 1
                    stats["converged"] += 1
                    break
            k += 1
        stats["steps"] = k
        if m == 0:
            return 0.0
        if converged:
            lo, hi = sn_multisect(a, b2, k, blo, bhi, 1e-6 if coarse_tol else 0.5 * (bhi - blo) / bhi, stats, **kw)
        else:
            lo = max(0.0, min(gmin, a_last - b_last))
            hi = max(gmax, a_last + b_last)
            lo, hi = sn_multisect(a, b2, k, lo, hi, tol_final, stats, **kw)
        return 0.5 * (lo + hi)


def sigma_model(W, stats=None, gram_f32=False, drop_tail=False, **kw):
    """float32 sigma_max of a float32 matrix as the chain computes it."""
    lmax = lambda_max(gram(W, gram_f32=gram_f32, drop_tail=drop_tail), stats, **kw)
    with np.errstate(invalid="ignore"):
        return np.float32(math.sqrt(max(lmax, 0.0)) if lmax == lmax else lmax)


VARIANTS = {
    "first_bracket": {"first_bracket": True},
    "first_check_8": {"first_check": 8},
    "gram_f32": {"gram_f32": True},
    "drop_tail": {"drop_tail": True},
    "no_zero_convention": {"no_zero_convention": True},
    "coarse_tol": {"coarse_tol": True},
    "no_prescale": {"prescale": False},       # the chain before sn_scale: overflows near the top of float32
}


def sigma_ref(W):
    """The two largest singular values of the float32 matrix by the fp64 SVD (the second 0 if there is none)."""
    s = np.linalg.svd(np.asarray(W, np.float64), compute_uv=False)
    return float(s[0]), float(s[1]) if s.size > 1 else 0.0


def ulp_err(sig, ref):
    """(sig - float32(ref)) in units of spacing(float32(ref)); 0 when both are 0."""
    r32 = np.float32(ref)
    d = float(np.float32(sig)) - float(r32)
    return 0.0 if d == 0.0 else d / float(np.spacing(r32))


def scale_of(sig32, ln_lambda):
    """scale = fmaxf(1, sigma32 / ln_lambda) in float32 (NaN / 1 -> 1 as fmaxf)."""
    with np.errstate(all="ignore"):
        q = np.float32(sig32) / np.float32(ln_lambda)
    return np.float32(1.0) if not (q > np.float32(1.0)) else q


# ---- operand generators (seeded, float32) --------------------------------------------------------

def gaussian(rows, cols, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal((rows, cols)) * scale).astype(np.float32)


def _orth(n, k, rng):
    q, _ = np.linalg.qr(rng.standard_normal((n, k)))
    return q


def from_spectrum(rows, cols, svals, seed):
    """U diag(svals) V^T with seeded orthonormal factors (fp64), rounded to float32."""
    rng = np.random.default_rng(seed)
    s = np.asarray(svals, np.float64)
    return ((_orth(rows, s.size, rng) * s) @ _orth(cols, s.size, rng).T).astype(np.float32)


SHAPES = [(1, 1), (1, 300), (300, 1), (2, 2), (7, 3), (16, 16), (23, 64), (24, 64), (25, 64), (100, 37), (127, 129),
          (129, 127), (128, 128), (198, 128), (1152, 64), (128, 1), (128, 17), (128, 31), (128, 33), (128, 511),
          (128, 513), (128, 1152), (17, 4000)]


def family_a():
    return {f"{r}x{c}": gaussian(r, c, 1000 + i, 1.0 / math.sqrt(max(r, c))) for i, (r, c) in enumerate(SHAPES)}


def _tail(n, top=0.9):
    return np.linspace(top, 0.05, n)


def family_b():
    out = {}
    for (r, c) in ((128, 1152), (128, 300)):
        def put(name, top, seed):
            s = np.concatenate([top, _tail(r - len(top), 0.9 * float(np.min(top)))])
            out[f"{name}_{c}"] = from_spectrum(r, c, s, seed)
        for e in range(1, 9):
            put(f"gap1e-{e}", np.array([1.0, 1.0 - 10.0 ** -e]), 2000 + e)
        for mult in (2, 3, 8):
            put(f"mult{mult}", np.ones(mult), 2010 + mult)
        put("cluster20x1e-4", 1.0 - 1e-4 * np.arange(21), 2020)
        put("cluster60x1e-3", 1.0 - 1e-3 * np.arange(61), 2021)
        out[f"flat0.99_{c}"] = from_spectrum(r, c, np.linspace(1.0, 0.99, r), 2022)
        out[f"flat0.999_{c}"] = from_spectrum(r, c, np.linspace(1.0, 0.999, r), 2023)
        for rank in (1, 2, 4, 23):
            out[f"rank{rank}_{c}"] = from_spectrum(r, c, np.linspace(1.0, 0.3, rank), 2030 + rank)
    # m < 24 and a Gershgorin interval 0.07 lambda_max wide: two rounds of a multisection to 1e-6 end 9e-7 wide
    out["flat0.98_12x64"] = from_spectrum(12, 64, 0.99 * np.linspace(1.0, 0.98, 12), 2040)
    return out


def family_c():
    out = {"identity128": np.eye(128, dtype=np.float32), "2I_128": 2 * np.eye(128, dtype=np.float32),
           "diag1..128": np.diag(np.arange(1, 129)).astype(np.float32),
           "diag1..20": np.diag(np.arange(1, 21)).astype(np.float32),
           "zero_128x300": np.zeros((128, 300), np.float32), "zero_7x3": np.zeros((7, 3), np.float32),
           "const_64x64": np.full((64, 64), 0.01, np.float32), "const_128x1152": np.full((128, 1152), 3.0, np.float32),
           "const_5x200": np.full((5, 200), -2.0, np.float32)}
    one = np.zeros((128, 300), np.float32)
    one[77, 123] = -3.5
    out["one_entry"] = one
    rng = np.random.default_rng(3000)
    for i, (r, c) in enumerate(((2, 2), (3, 5), (8, 8), (12, 40), (16, 16), (20, 7), (23, 23))):
        out[f"int_{r}x{c}"] = rng.integers(-3, 4, (r, c)).astype(np.float32)
    # the same integers far below unit scale: the 9 unscaled terms that open sturm_gt underflow to an exact
    # zero, the only way into sturm_gt_checked that a matrix can be built to take
    out["int_16x16_2^-72"] = out["int_16x16"] * np.float32(2.0 ** -72)
    out["int_23x23_2^-74"] = out["int_23x23"] * np.float32(2.0 ** -74)
    return out


SCALES = (1e-18, 1e-12, 1e-6, 1e6, 1e12, 1e17)


def family_d():
    base = gaussian(128, 576, 4000).astype(np.float64)
    out = {f"scale{s:g}": (base * s).astype(np.float32) for s in SCALES}
    # positive entries below 1 beside one column of 4096: in a float32 Gram every product of a split that
    # holds that column is lost against 2^24
    dom = np.random.default_rng(4003).uniform(0.5, 1.0, (128, 576)).astype(np.float32)
    dom[:, 0] = 4096.0
    out["dominant_column"] = dom
    return out


def d_companions():
    return {"7x3": gaussian(7, 3, 4001), "198x128": gaussian(198, 128, 4002, 0.1)}


def family_e(seeds=(0, 7, 1234)):
    """The U-Net's conv weights at init (128 bands, 36 x 36), as [rows, cols] float32 matrices."""
    import os
    import sys
    import torch
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.join(here, "golden"), here, os.path.join(os.path.dirname(here), "lrs-pnp-dip_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import dip_ref
    from gen_dip_golden import flat_params
    from lrspnp.dip import lipschitz_unet_units
    u = lipschitz_unet_units(128, 128, 128)
    offs, _ = dip_ref.param_offsets(u, 128, 36, 36)
    out = {}
    for seed in seeds:
        flat = torch.from_numpy(flat_params(u, seed, 128, 36, 36))
        for i in range(len(u)):
            W, *_ = dip_ref.views(flat, u, i, offs, 128, 36, 36)
            out[f"seed{seed}_node{i}"] = W.reshape(W.shape[0], -1).contiguous().numpy().astype(np.float32)
    return out


F_COMPONENTS = (1e-1, 1e-3, 1e-5, 0.0)
F_GAPS = (1e-2, 1e-3, 1e-4, 1e-5)


def aligned(c, gap, seed=5000, rows=128, cols=400, start=None):
    """rows x cols, sigma_1 = 1, sigma_2 = 1 - gap, the rest from 0.9 (1 - gap) down to 0.05; the top left
    singular vector has component c along the (normalised) start vector."""
    rng = np.random.default_rng(seed)
    s0 = start_vector(rows) if start is None else np.asarray(start, np.float64)
    s0 = s0 / np.linalg.norm(s0)
    w = rng.standard_normal(rows)
    w -= (w @ s0) * s0
    w /= np.linalg.norm(w)
    u1 = c * s0 + math.sqrt(1.0 - c * c) * w
    B = rng.standard_normal((rows, rows))
    B[:, 0] = u1
    U, R = np.linalg.qr(B)
    U[:, 0] *= np.sign(R[0, 0])
    sv = np.concatenate([[1.0, 1.0 - gap], _tail(rows - 2, 0.9 * (1.0 - gap))])
    return ((U * sv) @ _orth(cols, rows, rng).T).astype(np.float32)


def family_f():
    return {f"c{c:g}_g{g:g}": aligned(c, g, 5000 + 10 * i + j) for i, c in enumerate(F_COMPONENTS)
            for j, g in enumerate(F_GAPS)}


@functools.lru_cache(maxsize=None)
def contract_cases(with_e=True):
    """name -> matrix of every case of families A to E (E needs torch)."""
    out = {}
    for fam, cases in (("A", family_a()), ("B", family_b()), ("C", family_c()), ("D", family_d())):
        out.update({f"{fam}/{k}": v for k, v in cases.items()})
    if with_e:
        out.update({f"E/{k}": v for k, v in family_e().items()})
    return out

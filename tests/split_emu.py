"""CPU model of the split-bf16 product (csrc/lrs_split.h) and the operand sets of its accuracy tests.

Imported by tests/test_split_emu.py (CPU: the model's own checks and the proof that the GPU tests have
teeth) and tests/test_gpu_split_accuracy.py (the kernels against fp64 on the same operands).

The model: every fp32 operand is split into three bf16 terms (torch's round-to-nearest-even casts, each
remainder exact in fp32, as split_bf16), and a product is accumulated in fp32 once per plane pair and
32-k step, in split_mfma6's order.  What the matrix core does inside one such step (the 32 exact bf16
products and their sum) is taken as exact here; DESIGN.md §8.1 records what the hardware adds to that.

The tolerance of every test is 3 x the error of seq_fp32 (a plain fp32 GEMM: rank-1 updates in k order,
one rounding per fused multiply-add) on the same operands, in each metric; a degraded chain (a product of
the six lost, a two-way split, planes exchanged) must exceed it by 1.5 x in relative L2, which bounds the
inner length of every case at 576.
"""
import numpy as np
import torch
import torch.nn.functional as F

# ---- the split and the chains -------------------------------------------------------------------

def split3(x):
    """The three bf16 terms of an fp32 tensor, as fp32 tensors (split_bf16)."""
    x = torch.as_tensor(x, dtype=torch.float32)
    b0 = x.to(torch.bfloat16).float()
    r1 = x - b0
    b1 = r1.to(torch.bfloat16).float()
    b2 = (r1 - b1).to(torch.bfloat16).float()
    return b0, b1, b2


# split_mfma6's order (A plane, B plane): smallest terms first
SIX = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))
# each of the three i + j = 2 products dropped in turn
FIVE = tuple(tuple(p for p in SIX if p != d) for d in ((2, 0), (1, 1), (0, 2)))
THREE = tuple(p for p in SIX if p[0] + p[1] <= 1)
TWO_WAY = ((1, 1), (1, 0), (0, 1), (0, 0))   # with nsplit = 2


def chain(A, B, pairs, nsplit=3, kstep=32, swap_a=False):
    """A B accumulated in fp32, once per kstep and listed plane pair (in order).  nsplit = 2: a two-way
    split (two bf16 terms); swap_a: planes 1 and 2 of A exchanged (a staging site writing them swapped)."""
    A = torch.as_tensor(A, dtype=torch.float32)
    B = torch.as_tensor(B, dtype=torch.float32)
    pa = [p.double() for p in split3(A)[:nsplit]]
    pb = [p.double() for p in split3(B)[:nsplit]]
    if swap_a:
        pa[1], pa[2] = pa[2], pa[1]
    acc = torch.zeros(A.shape[0], B.shape[1], dtype=torch.float32)
    for k0 in range(0, A.shape[1], kstep):
        k1 = min(k0 + kstep, A.shape[1])
        for i, j in pairs:
            acc = (acc.double() + pa[i][:, k0:k1] @ pb[j][k0:k1]).float()
    return acc


# name -> chain: the degradations the GPU tests must be able to see
DEGRADED = {
    "FIVE[A_lo B_hi]": lambda A, B: chain(A, B, FIVE[0]),
    "FIVE[A_mid B_mid]": lambda A, B: chain(A, B, FIVE[1]),
    "FIVE[A_hi B_lo]": lambda A, B: chain(A, B, FIVE[2]),
    "SWAP_A": lambda A, B: chain(A, B, SIX, swap_a=True),
    "TWO_WAY": lambda A, B: chain(A, B, TWO_WAY, nsplit=2),
    "THREE": lambda A, B: chain(A, B, THREE),
}


def seq_fp32(A, B):
    """The plain fp32 GEMM that "fp32-GEMM accuracy" means: rank-1 updates in k order, the accumulator
    rounded to fp32 after every (fused) multiply-add."""
    A = torch.as_tensor(A, dtype=torch.float32).double()
    B = torch.as_tensor(B, dtype=torch.float32).double()
    acc = torch.zeros(A.shape[0], B.shape[1], dtype=torch.float32)
    for k in range(A.shape[1]):
        acc = (acc.double() + A[:, k:k + 1] * B[k:k + 1]).float()   # fp32 x fp32 is exact in fp64
    return acc


def reference(A, B):
    A = torch.as_tensor(A, dtype=torch.float32).double()
    B = torch.as_tensor(B, dtype=torch.float32).double()
    return A @ B, A.abs() @ B.abs()


def metrics(C, A, B, ref=None):
    """(relative L2, componentwise RMS of |err_ij| / (|A||B|)_ij over the entries with a non-zero
    denominator) of C against the fp64 product.  ref: reference(A, B), when the caller has it."""
    R, den = ref if ref is not None else reference(A, B)
    err = torch.as_tensor(C).double().reshape(R.shape) - R
    nz = den > 0
    return float(err.norm() / R.norm()), float((err[nz] / den[nz]).pow(2).mean().sqrt())


def row_rel(C, A, B, ref=None):
    """Relative L2 of every output row (rows whose reference is zero: 0)."""
    R, _ = ref if ref is not None else reference(A, B)
    err = torch.as_tensor(C).double().reshape(R.shape) - R
    n = R.norm(dim=1)
    return torch.where(n > 0, err.norm(dim=1) / n.clamp_min(1e-300), torch.zeros_like(n))


TOL_FACTOR = 3.0    # the tolerance: this many times seq_fp32's own error
SEPARATION = 1.5    # every degraded chain exceeds the tolerance by this factor (relative L2)
MAX_INNER = 576     # the longest inner length at which that separation holds


def tolerances(A, B, ref=None):
    """(tol relative L2, tol componentwise, tol per-row relative L2) = 3 x seq_fp32's error.  The per-row
    bound is 3 x the largest row error of seq_fp32 (the rows are exchangeable in relative terms)."""
    ref = ref if ref is not None else reference(A, B)
    S = seq_fp32(A, B)
    l2, cw = metrics(S, A, B, ref)
    return TOL_FACTOR * l2, TOL_FACTOR * cw, TOL_FACTOR * float(row_rel(S, A, B, ref).max())


def teeth_view(A, B, ncol=768):
    """The product the CPU teeth test evaluates: every row, and for a wide product an even subsample of
    ncol output columns (the error statistics do not depend on the column)."""
    if B.shape[1] <= ncol:
        return A, B
    idx = torch.linspace(0, B.shape[1] - 1, ncol).round().long()
    return A, B[:, idx].contiguous()


# ---- operand sets ---------------------------------------------------------------------------------
OPSETS = ("normal", "positive", "rowscale", "kscale")   # (a) (b) (c) (d); (e) is built from (a)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _draw(shape, opset, g):
    if opset == "positive":
        return torch.rand(shape, generator=g) + 0.5           # uniform 0.5 .. 1.5: no cancellation
    return torch.randn(shape, generator=g)


def _logspace(lo, hi, n, g=None):
    s = torch.logspace(lo, hi, n, dtype=torch.float64).float()
    return s if g is None else s[torch.randperm(n, generator=g)]   # shuffled: mixed inside one k-step


# ---- convs as GEMMs (fp64-exact im2col: upsample, then pad, then unfold) ---------------------------
def conv_gather(H, W, k, stride, pad, pm, up):
    """idx [k*k][P]: the source pixel (row-major in H x W) output pixel p reads through tap t, -1 = zero
    pad; and (Ho, Wo).  Built by running the reference's own pipeline on an image of pixel indices."""
    h = torch.arange(H * W, dtype=torch.float64).view(1, 1, H, W)
    if up:
        h = F.interpolate(h, scale_factor=2, mode="nearest")
    if pad:
        h = F.pad(h, (pad,) * 4, mode="reflect") if pm == 1 else F.pad(h, (pad,) * 4, value=-1.0)
    Ho, Wo = (h.shape[2] - k) // stride + 1, (h.shape[3] - k) // stride + 1
    return F.unfold(h, k, stride=stride)[0].long(), (Ho, Wo)


def conv_gemm(case, direction, x, w, b, gy):
    """(A, B) with A B = the conv's forward output [cout][P] (bias as one more inner index), its data
    gradient [cin][H W] or its weight gradient [cout][cin k k], all from the same gather table."""
    cin, cout, H, W, k, stride, pad, pm, up = case
    idx, (Ho, Wo) = conv_gather(H, W, k, stride, pad, pm, up)
    kk, P, Q = k * k, Ho * Wo, H * W
    if direction in ("fwd", "wgrad"):
        xz = torch.cat([x.reshape(cin, Q), torch.zeros(cin, 1)], 1)
        col = xz[:, torch.where(idx < 0, torch.full_like(idx, Q), idx)].reshape(cin * kk, P)
        if direction == "wgrad":
            return gy.reshape(cout, P).contiguous(), col.t().contiguous()
        A = torch.cat([w.reshape(cout, cin * kk), b.reshape(cout, 1)], 1)
        return A.contiguous(), torch.cat([col, torch.ones(1, P)], 0).contiguous()
    # data gradient: gx[c][q] = sum over (o, t, p with idx[t][p] == q) of w[o][c][t] gy[o][p]; the p of one
    # (t, q) fill `slots` inner indices (the rest read a zero column)
    idn = idx.numpy()
    lists = []
    slots = 1
    for t in range(kk):
        p = np.nonzero(idn[t] >= 0)[0]
        q = idn[t][p]
        order = np.argsort(q, kind="stable")
        p, q = p[order], q[order]
        first = np.searchsorted(q, q, side="left")
        rank = np.arange(q.size) - first
        lists.append((p, q, rank))
        slots = max(slots, int(rank.max()) + 1 if rank.size else 1)
    sl = np.full((kk, slots, Q), P, np.int64)
    for t, (p, q, rank) in enumerate(lists):
        sl[t, rank, q] = p
    gyz = torch.cat([gy.reshape(cout, P), torch.zeros(cout, 1)], 1)
    Bm = gyz[:, torch.from_numpy(sl)].reshape(cout * kk * slots, Q)
    A = w.reshape(cout, cin, kk).permute(1, 0, 2).unsqueeze(-1).expand(cin, cout, kk, slots).reshape(cin, -1)
    return A.contiguous(), Bm.contiguous()


def conv_inner(case, direction):
    """The inner length of that product (the non-zero terms of one output entry, at most)."""
    cin, cout, H, W, k, stride, pad, pm, up = case
    if direction == "fwd":
        return cin * k * k + 1
    if direction == "dgrad":
        return cout * k * k * (4 if up else 1)
    _, (Ho, Wo) = conv_gather(H, W, k, stride, pad, pm, up)
    return Ho * Wo


def conv_tensors(case, seed, opset, direction, scale=1.0):
    """x, w, bias, gy of one conv case, operand set and direction (the direction fixes which tensor the
    row / inner-index scalings of sets (c) and (d) act on).  scale (set (e)): the A-side tensor of the
    direction times scale, bias zero."""
    cin, cout, H, W, k, stride, pad, pm, up = case
    g = _gen(1000 * seed + 10 * OPSETS.index(opset if opset != "meta" else "normal"))
    _, (Ho, Wo) = conv_gather(H, W, k, stride, pad, pm, up)
    base = "normal" if opset == "meta" else opset
    x = _draw((cin, H, W), base, g)
    w = _draw((cout, cin, k, k), base, g) / float(np.sqrt(cin * k * k))
    b = _draw((cout,), base, g) * 0.1
    gy = _draw((cout, Ho, Wo), base, g)
    if opset == "rowscale":           # (c): the rows of A over 12 decades
        if direction == "fwd":
            s = _logspace(-6, 6, cout)
            w, b = w * s.view(-1, 1, 1, 1), b * s
        elif direction == "dgrad":
            w = w * _logspace(-6, 6, cin).view(1, -1, 1, 1)
        else:
            gy = gy * _logspace(-6, 6, cout).view(-1, 1, 1)
    elif opset == "kscale":           # (d): s on A's inner index, 1 / s on B's
        if direction == "fwd":
            s = _logspace(-3, 3, cin, g)
            w, x = w * s.view(1, -1, 1, 1), x / s.view(-1, 1, 1)
        elif direction == "dgrad":
            s = _logspace(-3, 3, cout, g)
            w, gy = w * s.view(-1, 1, 1, 1), gy / s.view(-1, 1, 1)
        else:                         # inner index = pixel: only a 1x1 conv's col is x itself
            assert k == 1 and stride == 1 and not up and not pad
            s = _logspace(-3, 3, H * W, g).view(1, H, W)
            gy, x = gy * s, x / s
    elif opset == "meta":
        b = torch.zeros_like(b)
        if direction == "wgrad":
            gy = gy * scale
        else:
            w = w * scale
    return x.contiguous(), w.contiguous(), b.contiguous(), gy.contiguous()


def conv_opsets(case, direction):
    k = case[4]
    plain = k == 1 and case[5] == 1 and case[6] == 0 and not case[8]
    return [o for o in OPSETS if not (o == "kscale" and direction == "wgrad" and not plain)]


# cin, cout, H, W, k, stride, pad, pad_mode, up -- and per case: the directions tested, whether it runs in
# the network engine (a two-node lrs_dipnet) instead of the conv primitives, and what it reaches.  The GPU
# test file repeats the kernel / loader pair next to each case.
CONV_CASES = {
    # conv primitives, col == NULL
    "s3_reflect":   ((32, 48, 19, 21, 3, 1, 1, 1, 0), ("fwd", "dgrad", "wgrad"), False),
    "s3_up3":       ((32, 16, 10, 11, 3, 1, 1, 1, 1), ("fwd", "dgrad", "wgrad"), False),
    "s3_up2":       ((32, 32, 9, 10, 2, 1, 0, 1, 1), ("fwd", "dgrad", "wgrad"), False),
    "s3_stride2":   ((32, 40, 21, 22, 3, 2, 1, 0, 0), ("fwd", "dgrad", "wgrad"), False),
    "s3_dense_tn":  ((32, 16, 108, 108, 3, 2, 1, 1, 0), ("fwd", "dgrad"), False),
    "s3_dense_nn":  ((32, 260, 52, 52, 1, 1, 0, 1, 0), ("fwd",), False),
    "pw_1x4":       ((48, 40, 20, 23, 1, 1, 0, 1, 0), ("fwd", "dgrad", "wgrad"), False),
    "pw_2x4":       ((100, 128, 20, 20, 1, 1, 0, 1, 0), ("fwd", "dgrad", "wgrad"), False),
    "pw_3x4":       ((64, 192, 16, 16, 1, 1, 0, 1, 0), ("fwd", "dgrad", "wgrad"), False),
    "pw_4x4":       ((37, 250, 9, 13, 1, 1, 0, 1, 0), ("fwd", "dgrad", "wgrad"), False),
    "pw_4x5":       ((16, 193, 196, 196, 1, 1, 0, 1, 0), ("fwd", "dgrad"), False),
    # network engine
    "sm_table":     ((32, 48, 9, 11, 3, 1, 1, 1, 0), ("fwd", "dgrad", "wgrad"), True),
    "sm_split":     ((32, 40, 19, 21, 3, 1, 1, 1, 0), ("fwd", "dgrad", "wgrad"), True),
    "upc":          ((32, 16, 16, 17, 3, 1, 1, 1, 1), ("fwd", "dgrad"), True),
}
POSITIVE_INNER = 32   # set (b): the longest inner length at which the separation holds


def case_for(name, direction, opset):
    """The shape a (case, direction, operand set) runs at, or None where it is left out.  Set (b) has
    no cancellation, so the reference grows like the inner length while a lost product still sums like its
    root: the 1.5 x separation holds up to an inner length of about 32 only.  Its cases keep the geometry (and so
    the kernel and the loader pair) and shorten the inner index: fewer input channels (forward), fewer
    output channels (data gradient), a map of at most 32 output pixels (weight gradient; left out where
    the path needs a larger map: the engine's sm_split and upc)."""
    case, _, engine = CONV_CASES[name]
    if opset != "positive":
        return case
    cin, cout, H, W, k, stride, pad, pm, up = case
    kk = k * k
    if direction == "fwd":
        cin = min(cin, (POSITIVE_INNER - 1) // kk)
    elif direction == "dgrad":   # (an upsampled conv's source pixel is read through 4 k k (output, tap) pairs)
        cout = max(1, min(cout, POSITIVE_INNER // (4 * kk if up else kk)))
    else:
        if engine and name != "sm_table":
            return None
        H, W = ((3, 3) if k == 2 else (2, 3)) if up else (9, 12) if stride == 2 else (5, 6)
    return (cin, cout, H, W, k, stride, pad, pm, up)


def conv_products():
    """Every (case name, direction, operand set) the GPU tests run."""
    return [(n, d, o) for n, (c, dirs, _) in CONV_CASES.items() for d in dirs for o in conv_opsets(c, d)
            if case_for(n, d, o) is not None]


def conv_operands(name, direction, opset, scale=1.0):
    """The shape, the tensors and the product (A, B) of one conv test."""
    case = case_for(name, direction, opset if opset != "meta" else "normal")
    x, w, b, gy = conv_tensors(case, list(CONV_CASES).index(name), opset, direction, scale)
    return case, (x, w, b, gy), conv_gemm(case, direction, x, w, b, gy)


# ---- dictionary learning: H = coefs^T coefs -------------------------------------------------------
# H's diagonal is a sum of squares (no cancellation) and carries most of ||H|| once nb > K, and set (c)
# leaves a few large columns to carry all of it: the separation then holds for shorter inner lengths only
# (measured in DESIGN.md 8.1), so nb = 500, and 256 beside K = 48, are reshaped to the lengths below.
# nb > 256 is k_dl_gemm's split-K path (dl_split: two chunks over gridDim.z, summed by k_dl_hrow): 288 =
# 160 + 128 and 300 = 160 + 140, the second chunk ragged and at 300 no multiple of the k-step; these are the
# reshaped nb = 500 (weakest degradation 1.45 x the tolerance there, 2.1 x at 288).
DICT_SHAPES = {"normal": [(37, 48), (130, 48), (37, 256), (130, 256), (256, 256), (288, 256), (300, 256)],
               "positive": [(19, 48), (32, 48), (19, 256), (32, 256)],
               "rowscale": [(37, 48), (70, 48), (37, 256), (70, 256)]}
DICT_OPSETS = tuple(DICT_SHAPES)


def dict_products():
    return [(nb, K, o) for o in DICT_OPSETS for nb, K in DICT_SHAPES[o]]


def dict_coefs(nb, K, opset):
    """Dense coefficients [nb][K]; set (c) scales their columns (the rows of A = coefs^T)."""
    g = _gen(7000 + 10 * nb + K + DICT_OPSETS.index(opset))
    A = _draw((nb, K), opset, g)
    if opset == "rowscale":
        A = A * _logspace(-6, 6, K).view(1, -1)
    return A.contiguous()


def dict_gemm(coefs):
    return coefs.t().contiguous(), coefs


# ---- ISTA: one soft-threshold iteration from x = 0 with T = 0 and alpha = 1 ------------------------
# (oracle/lrs_oracle.c oracle_ista_block: g = x + D^T (obs .* (y - D x)) / alpha; x = soft(g, T); phi = D x)
#   coefs = (obs .* Yb) D       [nb][n] x [n][K]
#   phi   = coefs D^T           [nb][K] x [K][n]
ISTA_N, ISTA_K, ISTA_NB = 64, 256, 130   # 64-block workgroups: two full and a ragged third
ISTA_OPSETS = ("normal", "positive")


def ista_inputs(opset):
    """Yb, obs [nb][n] and the synthetic dictionary D [n][K] (float32 tensors; obs uint8)."""
    from lrspnp.data import synthetic_dictionary
    g = _gen(9000 + ISTA_OPSETS.index(opset))
    D = torch.from_numpy(np.ascontiguousarray(synthetic_dictionary(ISTA_N, ISTA_K, 0), dtype=np.float32))
    Yb = _draw((ISTA_NB, ISTA_N), opset, g) * 0.3
    obs = (torch.rand((ISTA_NB, ISTA_N), generator=g) > 0.15).to(torch.uint8)
    return (Yb * obs).contiguous(), obs.contiguous(), D


ISTA_NPAT = 3


def ista_pat_inputs(opset):
    """The same blocks on three shared observation patterns (the first three rows of obs, cyclically):
    Yb, obs [nb][n], the patterns [npat][n], each block's pattern index (int32 numpy), D."""
    Yb, obs, D = ista_inputs(opset)
    pats = obs[:ISTA_NPAT].contiguous()
    pat = (np.arange(ISTA_NB) % ISTA_NPAT).astype(np.int32)
    obs2 = pats[torch.from_numpy(pat).long()].contiguous()
    return (Yb * obs2).contiguous(), obs2, pats, pat, D


ISTA_NLM_H = 0.1


def ista_nlm_coefs(opset):
    """The coefficients of one NLM-prox iteration from x = 0 (alpha = 1, h = 0.1) by the C oracle: the CPU
    stand-in for what k_ista_ln2 hands its second product."""
    from oracle import oracle as O
    Yb, obs, D = ista_inputs(opset)
    X, _ = O.ista_batch(Yb.numpy(), obs.numpy(), D.numpy(), np.ones(ISTA_NB, np.float32),
                        np.full(ISTA_NB, ISTA_NLM_H), 1, O.PROX_NLM)
    return torch.from_numpy(X), D


def ista_gemm_coefs(Yb, obs, D):
    return (Yb * obs).contiguous(), D.contiguous()


def ista_gemm_phi(coefs, D):
    return torch.as_tensor(coefs, dtype=torch.float32).contiguous(), D.t().contiguous()

"""CPU: the model of the split-bf16 product (tests/split_emu.py) and the proof that the GPU accuracy
tests (tests/test_gpu_split_accuracy.py) have teeth.

For every product those tests run (the same generators and seeds) the tolerance is 3 x the error of a
sequential fp32 GEMM; the six-product chain must be inside it in both metrics, and every degraded chain
(a dropped product, exchanged planes, a two-way split, three products) must exceed it by 1.5 x in
relative L2.  A wide product is evaluated on an even subsample of its output columns (teeth_view).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import split_emu as E  # noqa: E402


def _split_inputs():
    g = torch.Generator().manual_seed(11)
    wide = torch.randn(20000, generator=g) * torch.exp2(torch.rand(20000, generator=g) * 120 - 60)
    pow2 = torch.exp2(torch.arange(-100, 101, dtype=torch.float32))
    pow2 = torch.cat([pow2, -pow2])
    # one fp32 ulp below a bf16 rounding boundary (the midpoint of two neighbouring bf16 values)
    b = (torch.randn(4096, generator=g) * torch.exp2(torch.rand(4096, generator=g) * 40 - 20)).to(torch.bfloat16).float()
    mid = (b.view(torch.int32) + 0x8000).view(torch.float32)          # bf16 value + half a bf16 ulp: the boundary
    below = (mid.view(torch.int32) - 1).view(torch.float32)
    return {"wide": wide.float(), "pow2": pow2, "below_boundary": below}


@pytest.mark.parametrize("kind", ["wide", "pow2", "below_boundary"])
def test_split3_reconstructs(kind):
    x = _split_inputs()[kind]
    b0, b1, b2 = E.split3(x)
    for b in (b0, b1, b2):
        assert torch.equal(b, b.to(torch.bfloat16).float())            # every term is a bf16 value
    rec = b0.double() + b1.double() + b2.double()
    rel = ((rec - x.double()).abs() / x.double().abs()).max()
    assert float(rel) <= 2.0 ** -24
    if kind == "pow2":
        assert torch.equal(b0, x) and not b1.any() and not b2.any()
    if kind == "below_boundary":
        assert (b1 != 0).all()                                        # the remainder is the whole half ulp


def test_chain_orders():
    assert E.SIX == ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))
    assert all(len(f) == 5 for f in E.FIVE) and len({f for f in E.FIVE}) == 3
    assert set(E.THREE) == {(1, 0), (0, 1), (0, 0)}
    # bf16-exact operands: every chain that keeps A_hi B_hi is the exact product
    g = torch.Generator().manual_seed(3)
    A = torch.randint(-8, 9, (16, 40), generator=g).float()
    B = torch.randint(-8, 9, (40, 24), generator=g).float()
    assert torch.equal(E.chain(A, B, E.SIX), A @ B) and torch.equal(E.seq_fp32(A, B), A @ B)


def check_teeth(A, B, label, rows=False, separation=True):
    """separation=False (ISTA's phi): the six-product chain is held to the tolerance, the weakest
    degradation is printed, not asserted."""
    A, B = E.teeth_view(A, B)
    ref = E.reference(A, B)
    tol_l2, tol_cw, tol_row = E.tolerances(A, B, ref)
    C = E.chain(A, B, E.SIX)
    l2, cw = E.metrics(C, A, B, ref)
    worst = (None, np.inf)
    for name, fn in E.DEGRADED.items():
        d = E.metrics(fn(A, B), A, B, ref)[0]
        if d < worst[1]:
            worst = (name, d)
        assert not separation or d >= E.SEPARATION * tol_l2, f"{label}: {name} rel L2 {d:.3e} is not {E.SEPARATION} x tol {tol_l2:.3e}"
    print(f"{label}: inner {A.shape[1]}, SIX rel L2 {l2:.3e} (tol {tol_l2:.3e}), componentwise {cw:.3e} "
          f"(tol {tol_cw:.3e}); weakest degradation {worst[0]} {worst[1]:.3e} = {worst[1] / tol_l2:.2f} x tol")
    assert l2 <= tol_l2 and cw <= tol_cw
    if rows:
        r = float(E.row_rel(C, A, B, ref).max())
        assert r <= tol_row, f"{label}: worst row {r:.3e} > {tol_row:.3e}"
        for name, fn in E.DEGRADED.items():
            d = float(E.row_rel(fn(A, B), A, B, ref).max())
            assert d >= E.SEPARATION * tol_row, f"{label}: {name} worst row {d:.3e} vs tol {tol_row:.3e}"


@pytest.mark.parametrize("name,direction,opset", E.conv_products())
def test_conv_products_have_teeth(name, direction, opset):
    case, _, (A, B) = E.conv_operands(name, direction, opset)
    assert E.conv_inner(case, direction) <= (E.POSITIVE_INNER + 4 if opset == "positive" else E.MAX_INNER)  # +4: one channel of an upsampled 3x3 is 36
    check_teeth(A, B, f"{name} {direction} ({opset})", rows=opset == "rowscale")


@pytest.mark.parametrize("nb,K,opset", E.dict_products())
def test_dict_stats_products_have_teeth(nb, K, opset):
    assert nb <= (E.POSITIVE_INNER if opset == "positive" else E.MAX_INNER)
    A, B = E.dict_gemm(E.dict_coefs(nb, K, opset))
    check_teeth(A, B, f"dict_stats ({nb}, {K}) ({opset})")


# ISTA's phi = coefs D^T has K = 256 as its inner length, the only K the resident kernels serve, and
# coefs = Y D makes it nearly Y (D D^T): little cancellation, as H = A^T A.  Its weakest degradation is 1.46
# to 1.53 x the tolerance on every operand set (soft (a) 1.53, (b) 1.50; pattern kernel (a) 1.46, (b) 1.49; NLM (a) 1.52,
# (b) 1.46): on the edge of the 1.5 x condition and not reshapable, so the figure is printed and teeth are
# claimed for the first product only.  The GPU tests assert phi against the tolerance all the same.
@pytest.mark.parametrize("opset", E.ISTA_OPSETS)
def test_ista_products_have_teeth(opset):
    Yb, obs, D = E.ista_inputs(opset)
    A, B = E.ista_gemm_coefs(Yb, obs, D)
    check_teeth(A, B, f"ista coefs ({opset})")
    check_teeth(*E.ista_gemm_phi(E.seq_fp32(A, B), D), f"ista phi ({opset})", separation=False)


@pytest.mark.parametrize("opset", E.ISTA_OPSETS)
def test_ista_pat_products_have_teeth(opset):
    Y2, obs2, _, _, D = E.ista_pat_inputs(opset)
    A, B = E.ista_gemm_coefs(Y2, obs2, D)
    check_teeth(A, B, f"ista_pat coefs ({opset})")
    check_teeth(*E.ista_gemm_phi(E.seq_fp32(A, B), D), f"ista_pat phi ({opset})", separation=False)


@pytest.mark.parametrize("opset", E.ISTA_OPSETS)
def test_ista_nlm_phi_model(opset):
    """k_ista_ln2's second product on the C oracle's NLM-filtered coefficients."""
    X, D = E.ista_nlm_coefs(opset)
    check_teeth(*E.ista_gemm_phi(X, D), f"ista NLM phi ({opset})", separation=False)

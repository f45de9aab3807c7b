"""CPU: the fp64 model of the spectral-norm chain (tests/sn_emu.py) against numpy's fp64 SVD, and the proof
that the cases of tests/test_gpu_sigma.py have teeth.

Every contract case (families A to E, the matrices the GPU tests run) must come out within one float32 ulp
of the SVD of the same float32 matrix; every degraded variant of the model must miss by more than one ulp on
the case named beside it.  Family F (a top singular vector nearly orthogonal to the start vector) is where
the design itself can miss: the model's verdict per case is recorded in tests/golden/sn_f_verdicts.json,
checked here and read by the GPU test.
"""
import json
import os

import numpy as np
import pytest

import sn_emu as E

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("family", ["A", "B", "C", "D"])
def test_model_within_one_ulp(family):
    cases = {"A": E.family_a, "B": E.family_b, "C": E.family_c, "D": E.family_d}[family]()
    bad = {}
    for name, W in cases.items():
        u = E.ulp_err(E.sigma_model(W), E.sigma_ref(W)[0])
        if not abs(u) <= 1.0:
            bad[name] = u
    assert not bad, bad


def test_model_within_one_ulp_real_weights():
    pytest.importorskip("torch")
    bad = {}
    for name, W in E.family_e().items():
        u = E.ulp_err(E.sigma_model(W), E.sigma_ref(W)[0])
        if not abs(u) <= 1.0:
            bad[name] = u
    assert not bad, bad


def _case(name):
    fam, key = name.split("/")
    return {"A": E.family_a, "B": E.family_b, "C": E.family_c, "D": E.family_d, "F": E.family_f}[fam]()[key]


# variant -> the case on which it misses (the faithful model is within 1 ulp on every one of them; the F
# case is one of those the model gets right, and the GPU test holds the kernel to 1 ulp on it)
TEETH = {
    "first_bracket": "B/cluster20x1e-4_1152",
    "first_check_8": "F/c1e-05_g0.001",
    "gram_f32": "D/dominant_column",
    "drop_tail": "A/128x513",
    "no_zero_convention": "C/int_16x16_2^-72",
    "coarse_tol": "B/flat0.98_12x64",
    "no_prescale": "D/scale1e+17",
}


@pytest.mark.parametrize("variant", sorted(E.VARIANTS))
def test_variant_misses(variant):
    W = _case(TEETH[variant])
    ref = E.sigma_ref(W)[0]
    assert abs(E.ulp_err(E.sigma_model(W), ref)) <= 1.0
    u = E.ulp_err(E.sigma_model(W, **E.VARIANTS[variant]), ref)
    assert abs(u) > 1.0 or u != u, (variant, TEETH[variant], u)


def test_branches_reached():
    """The cases reach what they are there for (the model's step and branch counters)."""
    def stats(name):
        st = E.new_stats()
        E.sigma_model(_case(name), st)
        return st
    assert stats("C/int_16x16_2^-72")["checked"] > 0          # sturm_gt_checked
    assert stats("C/int_23x23_2^-74")["checked"] > 0
    st = stats("B/cluster20x1e-4_1152")
    assert st["steps"] >= 100 and st["rebracket"] >= 10 and st["moved"] >= 1 and st["converged"] == 1
    assert stats("B/rank2_300")["break"] == 1 and stats("B/rank2_300")["steps"] == 3
    assert stats("B/rank23_300")["checks"] >= 1                # rank 23: the first check sees an exact T
    for name in ("A/23x64", "A/24x64"):
        assert stats(name)["checks"] == 0 and stats(name)["exhausted"] == 1
    assert stats("A/25x64")["checks"] == 1
    assert stats("D/scale1e+17")["nonfinite"] == 0 and stats("D/scale1e-18")["checked"] == 0
    st = E.new_stats()
    E.sigma_model(_case("D/scale1e+17"), st, prescale=False)
    assert st["nonfinite"] > 0                                 # what sn_scale is for


def test_zero_nan_and_scale():
    assert E.sigma_model(np.zeros((7, 3), np.float32)) == 0.0
    assert E.scale_of(np.float32(0.0), 1.0) == 1.0
    assert E.scale_of(np.float32("nan"), 1.0) == 1.0           # fmaxf(1, NaN) = 1
    assert E.scale_of(np.float32(3.0), 2.0) == np.float32(1.5)
    assert E.scale_of(np.float32("inf"), 0.5) == np.float32("inf")


def test_family_f_verdicts_recorded():
    with open(os.path.join(HERE, "golden", "sn_f_verdicts.json")) as f:
        rec = json.load(f)
    cases = E.family_f()
    assert sorted(rec) == sorted(cases)
    for name, W in cases.items():
        s1, s2 = E.sigma_ref(W)
        sg = E.sigma_model(W)
        u = E.ulp_err(sg, s1)
        assert rec[name]["within_1ulp"] == (abs(u) <= 1.0), (name, u)
        assert rec[name]["model_ulp"] == u, (name, u)
        # never over the top, never worse than the gap
        assert sg <= np.float32(s1) + np.spacing(np.float32(s1))
        assert sg >= np.float32(s2) - np.spacing(np.float32(s2))
    # the hazard is real: an orthogonal start at gap 1e-3 settles on sigma_2
    assert not rec["c0_g0.001"]["within_1ulp"] and rec["c0.1_g1e-05"]["within_1ulp"]

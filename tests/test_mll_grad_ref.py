"""CPU tests of the MLL gradient's reference (tests/mll_grad_ref.py) and of the fit method's argument
checks: the long-double gradient against a central difference of exact_fit_ref's long-double MLL, its exact 0
at N = 1, the f64 restatement's error in units of the scale S (R, which the GPU tests hold the device to 8 x),
and the ValueErrors that need no device."""
import numpy as np
import pytest

import exact_fit_ref as F
import mll_grad_ref as G
from exact_ref import LD


@pytest.mark.parametrize("n", [2, 33, 65])
def test_reference_gradient_is_the_derivative_of_the_reference_mll(n):
    """Central differences of the long-double MLL in log l at h = 2e-3 and 1e-3 (the actual steps, after
    rounding l e^(+-h) to f64), Richardson-combined: the truncation left is h^4 / 30 times the fifth derivative,
    1e-13 of it, and the MLL's own long-double rounding divided by 2 h is 2^-11 u S_chol-like terms / 2e-3.  The
    derivatives of exp(-a) in log l are polynomials in a times exp(-a), of the size of D's entries, so both
    stay far below 1e-9 S."""
    p = F.mll_problem((n, 1e-8, ""))
    c = G.grad_case((n, 1e-8, ""))
    for o in range(3):
        ref = c["grefs"][o]
        est = []
        for h in (2e-3, 1e-3):
            lp, lm = float(p["ls"][o] * np.exp(h)), float(p["ls"][o] * np.exp(-h))
            step = np.log(LD(lp)) - np.log(LD(lm))
            fp = G.mll_ld(p["x"], p["y"][:, o], p["pm"][o], lp, 1e-8)
            fm = G.mll_ld(p["x"], p["y"][:, o], p["pm"][o], lm, 1e-8)
            est.append((fp - fm) / step)
        rich = (4 * est[1] - est[0]) / 3
        err = float(abs((rich - LD(ref["hi"])) - LD(ref["lo"])))
        print(f"N {n} objective {o}: g {ref['g']:.12g}, |difference quotient - g| / S {err / ref['S']:.2e}")
        assert err <= 1e-9 * ref["S"], (n, o, err, ref["S"])
        # the chain's own value is exact_fit_ref's
        assert abs(ref["mll"] - F.mll_case((n, 1e-8, ""))["refs"][o]["mll"]) <= 1e-12 * abs(ref["mll"])


def test_reference_gradient_is_zero_at_one_point():
    c = G.grad_case((1, 1e-8, ""))
    for o in range(3):
        assert c["grefs"][o]["hi"] == 0.0 and c["grefs"][o]["lo"] == 0.0 and c["grefs"][o]["S"] == 0.0
        assert c["restated"][o] == 0.0


def test_restatement_error_in_units_of_the_scale():
    """R: the largest err / (u S) of the f64 numpy restatement over the GPU tests' cases.  Computed, never
    hard-coded; R <= 1000 keeps a scale that stopped tracking the error from loosening the 8 R rule."""
    worst = {}
    for key in G.GRAD_CASES:
        c = G.grad_case(key)
        worst[key] = [G.grad_ratio(c["restated"][o], c["grefs"][o]) for o in range(3)]
        print(key, " ".join(f"{v:.3g}" for v in worst[key]))
    R = G.grad_R()
    print(f"R = {R:.4g}")
    assert R == max(max(v) for v in worst.values())
    assert np.isfinite(R) and 0.0 < R <= 1000.0


def test_scale_parts_are_positive_and_ordered():
    for key in G.GRAD_CASES:
        if key[0] == 1:
            continue
        for ref in G.grad_case(key)["grefs"]:
            assert ref["S_g"] > 0 and ref["S_p"] > 0 and ref["S"] == ref["S_g"] + ref["S_p"]
            assert abs(ref["g"]) <= ref["S_g"] * (1 + 1e-12)      # the sum of the terms' magnitudes bounds the sum


def test_fit_method_argument_checks():
    from bayesopt_smart_amd import config
    from bayesopt_smart_amd.bayesian_optimization import _check_limits
    from bayesopt_smart_amd.kernels import optimize_hyperparams_mll
    assert config.FIT_METHODS == ("powell", "lbfgs")
    for ok in config.FIT_METHODS:
        assert config.check_fit_method(ok) == ok
    with pytest.raises(ValueError, match="unknown fit method 'bogus'"):
        config.check_fit_method("bogus")
    # the constructor's check: first of all, before the library or a device is touched
    with pytest.raises(ValueError, match="unknown fit method 'bogus'"):
        _check_limits(2, 2, 64, 3, fit_method="bogus")
    with pytest.raises(ValueError, match="unknown fit method 'bogus'"):
        _check_limits(99, 2, 64, 3, fit_method="bogus")
    _check_limits(2, 2, 64, 3, fit_method="lbfgs")
    x, y = np.zeros((4, 2)), np.zeros((4, 2))
    with pytest.raises(ValueError, match="unknown fit method 'bogus'"):
        optimize_hyperparams_mll(x, y, np.zeros((2, 4, 4)), np.zeros(2), np.ones(2), np.ones(2), 4, method="bogus")


def test_numpy_fit_restatement_matches_the_reference_gradient():
    """mll_grad_ref.numpy_value_grad (the CPU fit used to choose the GPU fit test's problems) is the same
    quantity: its value and gradient agree with the long-double reference within 1e-9 of the scale."""
    key = (65, 1e-8, "")
    p, c = F.mll_problem(key), G.grad_case(key)
    v, g = G.numpy_value_grad(p["x"], p["y"], p["pm"], p["ls"])
    refs = F.mll_case(key)["refs"]
    consts = F.fit_constants("oracle", 65, p["dim"])       # LAPACK's unblocked Cholesky: exact_fit_ref's hard bound
    assert abs(v - sum(r["mll"] for r in refs)) <= sum(F.mll_tol(r, consts) for r in refs)
    for o in range(3):
        assert abs(g[o] - c["grefs"][o]["g"]) <= 1e-9 * c["grefs"][o]["S"]

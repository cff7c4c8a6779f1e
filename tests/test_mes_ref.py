"""tests/mes_ref.py pinned on the CPU: g against its definition (an entropy difference, by quadrature),
the f64 restatement of the device's three branches against the mpmath g under the rounding rule's unit,
and the limits of the reference acquisition."""
import mpmath as mp
import numpy as np
import pytest

import mes_ref as R


@pytest.mark.parametrize("x", [-8.0, -6.5, -5.0, -3.0, -1.5, -0.5, 0.0, 0.5, 1.5, 3.0, 5.0, 8.0])
def test_g_is_the_entropy_difference(x):
    want = R.entropy_difference_mp(x)
    got = R.g_mp(x)
    assert abs(got - want) <= mp.mpf(10) ** -12 * (1 + abs(want)), (x, got, want)


def test_g_shape():
    with mp.workdps(R.DPS):
        assert abs(R.g_mp(0.0) - mp.log(2)) < mp.mpf(10) ** -50
    xs = np.linspace(-30.0, 30.0, 121)
    g = [R.g_mp(x) for x in xs]
    assert all(v >= 0 for v in g) and all(a > b for a, b in zip(g, g[1:]))
    assert R.g_mp(np.inf) == 0 and R.g_mp(-np.inf) == mp.inf and mp.isnan(R.g_mp(np.nan))


def points():
    rng = np.random.default_rng(0)
    neg = -np.exp(rng.uniform(np.log(1e-9), np.log(1e8), 1200))
    pos = np.exp(rng.uniform(np.log(1e-9), np.log(40.0), 500))
    lin = np.linspace(-12.0, 40.0, 800)
    near = -0.003 + np.linspace(-0.003, 0.003, 41)
    cut = np.array([0.0, 1e-8, -1e-8, R.CUT, np.nextafter(R.CUT, 0.0), np.nextafter(R.CUT, -np.inf), -1e8, 40.0])
    return np.concatenate([neg, pos, lin, near, cut])


def test_f64_restatement_meets_16_units():
    xs = points()
    got = R.g_f64(xs)
    worst, at = 0.0, None
    for x, g in zip(xs, got):
        ref = R.g_mp(x)
        tol = R.C_F64 * float(R.unit(x, float(ref))) + R.TINY
        err = abs(float(mp.mpf(float(g)) - ref))
        if err / tol > worst:
            worst, at = err / tol, x
        assert err <= tol, (x, g, float(ref), err / tol)
    print("f64 restatement: worst error", worst * R.C_F64, "units of u (1 + x^2/2) g, at x =", at)


def test_f64_restatement_limits():
    g = R.g_f64(np.array([np.inf, -np.inf, np.nan, 0.0]))
    assert g[0] == 0.0 and g[1] == np.inf and np.isnan(g[2]) and abs(g[3] - np.log(2.0)) <= 2 * R.U


def test_reference_acquisition_limits():
    mu = np.array([[0.0, 1.0, 0.0, np.nan, 0.0, 0.0]])
    var = np.array([[0.0, 0.0, 1.0, 1.0, np.nan, -4.0]])
    ys = np.array([[0.5]])
    acq, bound = R.acquisition_ref(mu, var, ys)
    assert acq[0] == 0.0 and acq[1] == np.inf and np.isnan(acq[3]) and np.isnan(acq[4])
    assert abs(acq[2] - float(R.g_mp(0.5))) <= 1e-16 and bound[2] > 0
    assert abs(acq[5] - float(R.g_mp(0.25))) <= 1e-16            # sigma = sqrt(|var|)
    a, _ = R.acquisition_ref(mu[:, 2:3], var[:, 2:3], np.array([[np.inf]]))
    b, _ = R.acquisition_ref(mu[:, 2:3], var[:, 2:3], np.array([[-np.inf]]))
    c, _ = R.acquisition_ref(mu[:, 2:3], var[:, 2:3], np.array([[np.nan]]))
    assert a[0] == 0.0 and b[0] == np.inf and np.isnan(c[0])
    # NaN beats +inf, whatever the order of the terms
    d, _ = R.acquisition_ref(np.array([[0.0], [np.nan]]), np.array([[0.0], [1.0]]), np.array([[-1.0, 0.0]]))
    assert np.isnan(d[0])
    # the mean over S and the sum over the objectives
    e, _ = R.acquisition_ref(np.zeros((2, 1)), np.ones((2, 1)), np.array([[0.0, 1.0], [2.0, -1.0]]))
    want = (R.g_mp(0.0) + R.g_mp(1.0) + R.g_mp(2.0) + R.g_mp(-1.0)) / 2
    assert abs(e[0] - float(want)) <= 1e-15


def test_maxima_reference_and_selection_helper():
    p = np.array([[1.0, np.nan, 3.0, -np.inf], [np.nan, np.nan, np.nan, np.nan], [-0.0, -1.0, -2.0, -3.0]])
    y = R.maxima_ref(p, np.array([0.5]), np.array([2.0]))
    assert y[0] == 6.5 and np.isnan(y[1]) and y[2] == 0.5
    assert R.fma_once(3.0, 1.0 + 2.0 ** -52, -3.0) == 3.0 * 2.0 ** -52       # one rounding
    picks, gaps, nxt = R.select_top(np.array([1.0, 5.0, 3.0, 4.0, 2.0]), np.array([False, True, False, False, False]), 2)
    assert picks.tolist() == [3, 2] and gaps.tolist() == [1.0, 1.0] and nxt.tolist() == [2, 4]

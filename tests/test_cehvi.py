"""Outcome constraints (the feasibility-weighted EHVI; not in the reference: PARITY UNPINNED), the
part that needs no GPU: the numpy probability of feasibility of tests/cehvi_ref.py against mpmath
at 60 digits, the numpy constrained EHVI against a Monte-Carlo mean, the limits, the feasibility
helper, bo_constrained_ehvi's argument checks and the loop's validation messages."""
import ctypes

import numpy as np
import pytest

import cehvi_ref as C
import ehvi_ref as R
from oracle import oracle_np as O
from test_ehvi import _hvi_from_boxes_chunked
from test_hvi import _front

N_DRAWS = 200_000
N_POSTERIORS = 10
N_POF_CASES = 4000                   # per seed


def _pof_cases(seed, n=N_POF_CASES):
    """mu ~ 3 N(0, 1), sigma log-uniform in [1e-3, 5], lo ~ 3 N(0, 1), hi - lo log-uniform in
    [1e-6, 20]; a third of the cases one-sided below (lo = -inf), a third one-sided above."""
    rng = np.random.default_rng(seed)
    mu = 3.0 * rng.standard_normal(n)
    sigma = np.exp(rng.uniform(np.log(1e-3), np.log(5.0), n))
    lo = 3.0 * rng.standard_normal(n)
    hi = lo + np.exp(rng.uniform(np.log(1e-6), np.log(20.0), n))
    side = np.arange(n) % 3
    lo = np.where(side == 1, -np.inf, lo)
    hi = np.where(side == 2, np.inf, hi)
    return mu, sigma, lo, hi


def _pof_mp(mu, sigma, lo, hi):
    """P(lo <= Y <= hi) at 60 digits from the doubles given, in the flipped tail form (ncdf(30) is
    exactly 1 at any practical precision, so Phi(zb) - Phi(za) would say nothing in the tails)."""
    import mpmath as mp
    mp.mp.dps = 60
    s2 = mp.sqrt(2)

    def q(z):
        return mp.erfc(z / s2) / 2

    mu, sigma = mp.mpf(float(mu)), mp.mpf(float(sigma))
    za = mp.mpf("-inf") if lo == -np.inf else (mp.mpf(float(lo)) - mu) / sigma
    zb = mp.mpf("inf") if hi == np.inf else (mp.mpf(float(hi)) - mu) / sigma
    if za > 0:
        return q(za) - q(zb)
    if zb < 0:
        return q(-zb) - q(-za)
    return 1 - q(zb) - q(-za)


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_pof_matches_extended_precision(seed):
    """|pof - exact| <= (8 z^2 + 32) u T per case, u = 2^-53, T the larger positive term (1 in the
    central branch), z its argument (0 there): z carries about 3 u of relative error from the
    subtraction, the division and the scaling by 1 / sqrt 2, the tail's logarithmic derivative is
    about z (so 3 z^2 u), erfc adds a few ulps; the factor 8 leaves scipy's erfc at well under the
    bound.  Cases with T < 1e-300 (the tail near the underflow) are skipped, at most 35 % of them."""
    import mpmath as mp
    mu, sigma, lo, hi = _pof_cases(seed)
    got, big, _ = C.pof_terms(mu, sigma, lo, hi)
    bound = C.pof_bound(mu, sigma, lo, hi)
    use = big >= 1e-300
    assert np.count_nonzero(~use) <= 0.35 * use.size
    worst = 0.0
    for i in np.flatnonzero(use):
        err = abs(float(_pof_mp(mu[i], sigma[i], lo[i], hi[i]) - mp.mpf(float(got[i]))))
        worst = max(worst, err / bound[i])
        assert err <= bound[i], (mu[i], sigma[i], lo[i], hi[i], got[i], err, bound[i])
    print(f"seed {seed}: {np.count_nonzero(use)} cases used, {np.count_nonzero(~use)} skipped, "
          f"worst error / bound = {worst:.3f}")


# constraint c: bounds and the range of its posterior (mean, sigma); chosen so that the joint
# probability of feasibility stays above a few per cent and the Monte-Carlo mean has support
_MC_BOUNDS = np.array([[-0.5, np.inf], [-1.0, 1.5]])


@pytest.mark.parametrize("m,c,n", [(m, c, n) for m in (1, 2, 3) for c in (1, 2) for n in (0, 5)])
def test_reference_matches_monte_carlo(m, c, n):
    """|cehvi - MC mean of HVI(Y_obj) 1{feasible(Y_con)}| <= 5 standard errors of that mean, for 10
    random posteriors per case out of at most 200 tried; one is used only when at least 50 of its
    2e5 draws are both feasible and improving (tests/test_ehvi.py's rule)."""
    from bayesopt_smart_amd.acquisition import hypervolume_boxes
    rng = np.random.default_rng(5000 + 100 * m + 10 * c + n)
    front = _front(rng, n, m, "cont")
    boxes = hypervolume_boxes(front, np.full(m, -1.0))
    bounds = _MC_BOUNDS[:c]
    z = rng.standard_normal((N_DRAWS, m + c))
    used, worst = 0, 0.0
    for _ in range(20 * N_POSTERIORS):
        mu = np.concatenate([rng.uniform(-1.0, 6.0, size=m), rng.uniform(-1.0, 1.0, size=c)])
        sigma = np.concatenate([rng.uniform(0.05, 2.0, size=m), rng.uniform(0.3, 1.5, size=c)])
        y = mu + sigma * z
        val = _hvi_from_boxes_chunked(boxes, y[:, :m]) * C.feasible(y, m, bounds)
        if np.count_nonzero(val) < 50:
            continue
        ref = C.cehvi(mu[:, None], (sigma ** 2)[:, None], boxes, bounds)[0]
        se = val.std(ddof=1) / np.sqrt(N_DRAWS)
        dev = abs(ref - val.mean()) / se
        worst = max(worst, dev)
        assert dev <= 5.0, (mu, sigma, ref, val.mean(), se)
        used += 1
        if used == N_POSTERIORS:
            break
    assert used == N_POSTERIORS
    print(f"m={m} c={c} n={n}: worst deviation {worst:.2f} standard errors")


def test_pof_limits():
    inf = np.inf
    # sigma = 0: inside, outside (both sides) and on either bound
    mu = np.array([0.5, -2.0, 3.0, 0.0, 1.0])
    assert np.array_equal(C.pof(mu, np.zeros(5), 0.0, 1.0), [1.0, 0.0, 0.0, 1.0, 1.0])
    # (-inf, +inf) is exactly 1, with any posterior
    assert np.array_equal(C.pof(np.array([0.3, -50.0, 1e300]), np.array([1.0, 1e-3, 0.0]), -inf, inf), np.ones(3))
    # NaN in mu or sigma
    assert np.isnan(C.pof(np.array([np.nan, 0.0, np.nan]), np.array([1.0, np.nan, 0.0]), -1.0, 1.0)).all()
    # both tails keep their digits: symmetric intervals mirror exactly, and far tails are ordered
    a = C.pof(np.array([0.0]), np.array([1.0]), 12.0, 13.0)[0]
    b = C.pof(np.array([0.0]), np.array([1.0]), -13.0, -12.0)[0]
    assert a == b and 0.0 < a < 1e-30
    assert C.pof(np.array([0.0]), np.array([1.0]), 13.0, inf)[0] < a
    assert C.pof(np.array([0.0]), np.array([1.0]), 45.0, inf)[0] == 0.0
    # no constraints: the plain closed form
    mu2, var2 = np.array([[0.3, 1.0]]), np.array([[1.0, 2.0]])
    boxes = np.array([[0.0, inf]])
    assert np.array_equal(C.cehvi(mu2, var2, boxes, np.zeros((0, 2))), R.ehvi(mu2, var2, boxes))


def test_feasible_front_leaves_out_a_dominating_infeasible_row():
    from bayesopt_smart_amd.acquisition import check_constraint_bounds, feasible_rows
    #             objectives   constraint (feasible in [0, 1])
    y = np.array([[9.0, 9.0, 2.0],          # dominates every other row, infeasible
                  [1.0, 3.0, 0.0],          # on the lower bound: feasible
                  [3.0, 1.0, 1.0],          # on the upper bound: feasible
                  [0.5, 0.5, 0.5],          # feasible, dominated
                  [4.0, 4.0, np.nan]])      # a NaN constraint value is infeasible
    bounds = [(0.0, 1.0)]
    ok = feasible_rows(y, 2, bounds)
    assert np.array_equal(ok, [False, True, True, True, False])
    assert np.array_equal(ok, C.feasible(y, 2, bounds))
    obj = y[ok][:, :2]
    front = obj[O.is_pareto_efficient(obj)]
    assert np.array_equal(front, [[1.0, 3.0], [3.0, 1.0]])
    assert O.is_pareto_efficient(y[:, :2]).tolist() == [True, False, False, False, False]
    # one-sided bounds, and the bounds' own rules
    assert np.array_equal(feasible_rows(y, 2, [(-np.inf, 0.5)]), [False, True, False, True, False])
    assert check_constraint_bounds([(0.0, 1.0), (-np.inf, np.inf)], 2).shape == (2, 2)
    for bad, why in (([(1.0, 0.0)], "exceeds"), ([(np.nan, 0.0)], "NaN"), ([(0.0, np.nan)], "NaN"),
                     ([(np.inf, np.inf)], "inf"), ([(-np.inf, -np.inf)], "inf")):
        with pytest.raises(ValueError, match=why):
            check_constraint_bounds(bad)
    with pytest.raises(ValueError, match="one .* pair per constraint"):
        check_constraint_bounds([(0.0, 1.0)], 2)


def test_scan_argument_checks_return_before_the_device():
    """Every call here returns from the argument checks, before any HIP call: the device arrays are
    NULL or never dereferenced."""
    from bayesopt_smart_amd import _lib
    lib = _lib.load()
    f = lib.bo_constrained_ehvi
    assert f.argtypes is not None and len(f.argtypes) == 17 and f.restype is ctypes.c_int
    ne = (ctypes.c_int32 * 4)(1, 1, 1, 1)
    p = 4096                                                # never dereferenced
    inf, nan = np.inf, np.nan

    def call(n_obj, n_con, lo, hi, acq=None, n=8):
        lo_a = (ctypes.c_double * max(len(lo), 1))(*lo) if lo is not None else None
        hi_a = (ctypes.c_double * max(len(hi), 1))(*hi) if hi is not None else None
        return f(acq, None, None, None, 8, n, n_obj, n_con, lo_a, hi_a, None, 1, None, ne, None, 0, None)

    assert call(2, 1, [1.0], [0.0]) == _lib.ERR_ARG                 # lo > hi
    assert call(2, 1, [nan], [0.0]) == _lib.ERR_ARG                 # a NaN bound
    assert call(2, 1, [0.0], [nan]) == _lib.ERR_ARG
    assert call(2, 1, [inf], [inf]) == _lib.ERR_ARG                 # lo = +inf
    assert call(2, 1, [-inf], [-inf]) == _lib.ERR_ARG               # hi = -inf
    assert call(2, 2, [0.0, 1.0], [1.0, 0.5]) == _lib.ERR_ARG       # the second pair
    assert call(0, 1, [0.0], [1.0]) == _lib.ERR_ARG                 # n_obj outside 1..4
    assert call(5, 1, [0.0], [1.0]) == _lib.ERR_ARG
    assert call(2, -1, [0.0], [1.0]) == _lib.ERR_ARG                # n_con < 0
    assert call(4, 5, [0.0] * 5, [1.0] * 5) == _lib.ERR_ARG         # n_obj + n_con > BO_MAX_OBJ
    assert call(2, 1, None, [1.0]) == _lib.ERR_ARG                  # no bounds
    assert call(2, 1, [0.0], None) == _lib.ERR_ARG
    # good bounds reach the scan's own checks: NULL arrays are refused there, still before the device
    assert call(2, 1, [0.0], [1.0]) == _lib.ERR_ARG
    assert call(4, 4, [-inf] * 4, [inf] * 4) == _lib.ERR_ARG
    # ... and with arrays (never dereferenced: n = 0) every check passes
    lo_a, hi_a = (ctypes.c_double * 1)(0.0), (ctypes.c_double * 1)(0.0)       # lo = hi is allowed
    assert f(p, p, p, p, 8, 0, 2, 1, lo_a, hi_a, p, 1, p, ne, p, 0, None) == _lib.OK
    assert f(p, None, p, p, 8, 0, 2, 0, None, None, p, 1, p, ne, p, 0, None) == _lib.OK
    assert f(p, p, p, p, 7, 8, 2, 1, lo_a, hi_a, p, 1, p, ne, p, 0, None) == _lib.ERR_ARG     # ld < n


def test_validation_messages(monkeypatch):
    from bayesopt_smart_amd import distributed
    from bayesopt_smart_amd.bayesian_optimization import _check_limits
    ok = dict(n_constraints=1, constraint_bounds=[(0.0, np.inf)])
    _check_limits(2, 2, 64, 3, "ehvi", "top", **ok)
    _check_limits(4, 2, 64, 3, "ehvi", "top", n_constraints=4, constraint_bounds=[(0.0, 1.0)] * 4)
    _check_limits(2, 2, 64, 3, "ehvi", "kb")                       # without constraints: as before
    with pytest.raises(ValueError, match=r"need acquisition='ehvi'.*'sum_ucb' takes negative values"):
        _check_limits(2, 2, 64, 3, "sum_ucb", "top", **ok)
    with pytest.raises(ValueError, match=r"need acquisition='ehvi'.*'hvi' scores UCB vectors"):
        _check_limits(2, 2, 64, 3, "hvi", "top", **ok)
    with pytest.raises(ValueError, match=r"need batch_strategy='top'.*'kb' would have to condition"):
        _check_limits(2, 2, 64, 3, "ehvi", "kb", **ok)
    with pytest.raises(ValueError, match=r"need batch_strategy='top'.*'ts' would have to sample"):
        _check_limits(2, 2, 64, 3, "ehvi", "ts", **ok)
    with pytest.raises(ValueError, match=r"need batch_strategy='top'.*'bucb' is not defined for the EHVI"):
        _check_limits(2, 2, 64, 3, "ehvi", "bucb", **ok)
    with pytest.raises(ValueError, match=r"1 <= n_objectives <= 4 \(got 5\)"):
        _check_limits(5, 2, 64, 3, "ehvi", "top", **ok)
    with pytest.raises(ValueError, match=r"n_objectives \+ n_constraints must be <= 8 \(got 4 \+ 5\)"):
        _check_limits(4, 2, 64, 3, "ehvi", "top", n_constraints=5, constraint_bounds=[(0.0, 1.0)] * 5)
    with pytest.raises(ValueError, match="one .* pair per constraint: got 1 for n_constraints=2"):
        _check_limits(2, 2, 64, 3, "ehvi", "top", n_constraints=2, constraint_bounds=[(0.0, 1.0)])
    with pytest.raises(ValueError, match="one .* pair per constraint: got 0 for n_constraints=1"):
        _check_limits(2, 2, 64, 3, "ehvi", "top", n_constraints=1)
    with pytest.raises(ValueError, match="one .* pair per constraint: got 1 for n_constraints=0"):
        _check_limits(2, 2, 64, 3, "ehvi", "top", constraint_bounds=[(0.0, 1.0)])
    with pytest.raises(ValueError, match="n_constraints must be >= 0"):
        _check_limits(2, 2, 64, 3, "ehvi", "top", n_constraints=-1)
    with pytest.raises(ValueError, match="constraint 0: the lower bound 1.0 exceeds the upper bound 0.0"):
        _check_limits(2, 2, 64, 3, "ehvi", "top", n_constraints=1, constraint_bounds=[(1.0, 0.0)])
    with pytest.raises(ValueError, match="constraint 1: a bound is NaN"):
        _check_limits(2, 2, 64, 3, "ehvi", "top", n_constraints=2, constraint_bounds=[(0.0, 1.0), (np.nan, 1.0)])
    with pytest.raises(ValueError, match=r"lo = \+inf or hi = -inf"):
        _check_limits(2, 2, 64, 3, "ehvi", "top", n_constraints=1, constraint_bounds=[(-np.inf, -np.inf)])
    # several ranks: constraints run as "ehvi" does; "kb" is refused for the constraints' reason
    monkeypatch.setattr(distributed, "collectives_on", lambda group=None: True)
    _check_limits(2, 2, 64, 3, "ehvi", "top", **ok)
    with pytest.raises(ValueError, match=r"need batch_strategy='top'.*'kb'"):
        _check_limits(2, 2, 64, 3, "ehvi", "kb", **ok)
    with pytest.raises(ValueError, match="one rank"):              # the existing message, word for word
        _check_limits(2, 2, 64, 3, "ehvi", "kb")


def test_constructor_length_checks(monkeypatch):
    """The constructor's checks run before the objective is evaluated and before a device buffer is
    allocated (the device lookup is replaced: this test has no GPU)."""
    import torch
    from bayesopt_smart_amd import bayesian_optimization as B
    monkeypatch.setattr(B, "require_device", lambda device=None: torch.device("cpu"))
    calls = []

    def fn(x):
        calls.append(x)
        return np.zeros(3)

    kw = dict(n_objectives=2, n_constraints=1, constraint_bounds=[(0.0, np.inf)], acquisition="ehvi",
              initial_samples=4, n_iterations=1, batch_size=2)
    with pytest.raises(ValueError, match=r"prior_mean must have one entry per output.*= 3 \(got 2\)"):
        B.BayesianOptimization(fn, [(0, 8), (0, 8)], **kw, prior_mean=[0.0, 0.0])
    with pytest.raises(ValueError, match=r"betas must have one entry per output.*= 3 \(got 4\)"):
        B.BayesianOptimization(fn, [(0, 8), (0, 8)], **kw, betas=[1.0] * 4)
    with pytest.raises(ValueError, match=r"reference_point must have one coordinate per objective.*= 2 \(got 3\)"):
        B.BayesianOptimization(fn, [(0, 8), (0, 8)], **kw, reference_point=[0.0, 0.0, 0.0])
    with pytest.raises(ValueError, match="one .* pair per constraint: got 2 for n_constraints=1"):
        B.BayesianOptimization(fn, [(0, 8), (0, 8)], **{**kw, "constraint_bounds": [(0.0, 1.0), (0.0, 1.0)]})
    with pytest.raises(ValueError, match="need acquisition='ehvi'"):
        B.BayesianOptimization(fn, [(0, 8), (0, 8)], **{**kw, "acquisition": "sum_ucb"})
    assert not calls

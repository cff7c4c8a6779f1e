"""The GIBBON batch in numpy alone (tests/gibbon_ref.py): the log-determinant identity the penalty
rests on, the spread of the batch, and the documented failure of the plug-in form.  No device, no
library -- but the strategy these statements are about must exist in the package."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bucb_ref as R          # noqa: E402
import gibbon_ref as G        # noqa: E402

PV = np.array([1.3, 0.7, 1.1])
LS = np.array([4.0, 6.0, 5.0])
SEED, N_TRAIN, Q = 3, 24, 5


@pytest.fixture(scope="module", autouse=True)
def strategy_exists():
    from bayesopt_smart_amd import acquisition
    assert "gibbon" in acquisition.MES_BATCH_STRATEGIES


def grid_points(lo, shape):
    ax = [np.arange(a, a + s) for a, s in zip(lo, shape)]
    return np.stack([m.ravel() for m in np.meshgrid(*ax, indexing="ij")], axis=-1).astype(np.float64)


def smooth_y(rng, x, n_obj, span):
    y = np.empty((x.shape[0], n_obj))
    for o in range(n_obj):
        w = rng.uniform(0.6, 1.6, x.shape[1]) * 2 * np.pi / span
        ph = rng.uniform(0, 2 * np.pi, x.shape[1])
        y[:, o] = np.sin(x * w + ph).sum(axis=1) + 0.05 * rng.standard_normal(x.shape[0])
    return y


def case(jitter, n_obj=3, seed=SEED, n_s=4, entropy=True):
    """33 x 31 grid, 24 training points; base = the max-value entropy over exact joint draws
    (`entropy` False: the summed variance, any deterministic array will do)."""
    pts = grid_points((-5, 100), (33, 31))
    x = pts[np.random.default_rng(seed).choice(pts.shape[0], N_TRAIN, replace=False)]
    y = smooth_y(np.random.default_rng(seed + 1000), x, n_obj, 32.0)
    pm, pv, ls = y.mean(axis=0), PV[:n_obj], LS[:n_obj]
    excluded = (pts[:, None, :] == x[None, :, :]).all(-1).any(-1)
    mu = cov = ystar = None
    if entropy:
        mu, cov = G.posterior_mean_cov(x, y, pts, pm, pv, ls, jitter)
        var = np.maximum(np.einsum("oii->oi", cov), 1e-10)
        ystar = G.sampled_maxima(mu, cov, n_s, seed + 2000)
        base = G.mes(mu, var, ystar)
    else:
        base = R.posterior(x, y, pts, pm, pv, ls, jitter, 1e-10)[1].sum(axis=0)
    ref = G.gibbon_reference(x, y, pts, pm, pv, ls, jitter, 1e-10, Q, excluded, base)
    return dict(pts=pts, x=x, y=y, pm=pm, pv=pv, ls=ls, jitter=jitter, mu=mu, cov=cov, ystar=ystar, base=base,
                excluded=excluded, ref=ref)


@pytest.fixture(scope="module")
def c6():
    return case(1e-6)


def penalty_sum(c, lam=0.0):
    """sum_t log((var^(t-1)(p_t) + lam) / (var^0(p_t) + lam)) per objective, from the reference's
    own augmented-Gram variances."""
    idx = c["ref"]["idx"]
    tot = np.zeros(len(c["pv"]))
    for t, p in enumerate(idx):
        _, var = R.posterior(c["x"], c["y"], c["pts"], c["pm"], c["pv"], c["ls"], c["jitter"], 0.0,
                             extra=c["pts"][idx[:t]])
        tot += np.log((var[:, p] + lam) / (c["ref"]["var0"][:, p] + lam))
    return tot


def log_det_correlation(cov, lam=0.0):
    s = cov + lam * np.eye(cov.shape[0])
    d = np.sqrt(np.diag(s))
    return np.linalg.slogdet(s / d[:, None] / d[None, :])[1]


def batch_cov(c):
    """The posterior covariance [n_obj, q, q] among the batch's points, computed directly."""
    return G.posterior_mean_cov(c["x"], c["y"], c["pts"][c["ref"]["idx"]], c["pm"], c["pv"], c["ls"], c["jitter"])[1]


def test_log_det_identity(c6):
    """sum_t log(var^(t-1)(p_t) / var^0(p_t)) = log det R, R the predictive correlation matrix of the
    batch computed directly from the posterior covariance.  The hallucinated observations carry the
    jitter lam, so the Schur chain is exact for (var + lam) and the matrix Sigma + lam I:
      * with the loop's lam = 1e-6 that exact form holds to 1e-8 relative;
      * the form the penalty uses (no lam) differs from it by O(lam / var) per term, so it is held
        to 1e-8 relative where lam is small enough for that: lam = 1e-12 (the test asserts that
        numpy's inverse of K + lam I is still accurate on these 24 distinct grid points)."""
    cov, tot = batch_cov(c6), penalty_sum(c6, 1e-6)
    for o in range(3):
        direct = log_det_correlation(cov[o], 1e-6)
        got = tot[o]
        assert direct < -1e-3                                           # a batch with correlation to penalise
        assert abs(got - direct) <= 1e-8 * abs(direct), (o, got, direct)
    c = case(1e-12, entropy=False)
    cov, tot = batch_cov(c), penalty_sum(c)
    for o in range(3):
        k = R.rbf(c["x"], c["x"], c["pv"][o], c["ls"][o]) + 1e-12 * np.eye(N_TRAIN)
        assert np.abs(np.linalg.inv(k) @ k - np.eye(N_TRAIN)).max() < 1e-7
        direct = log_det_correlation(cov[o])
        got = tot[o]
        assert abs(got - direct) <= 1e-8 * abs(direct), (o, got, direct)


def test_first_pick_and_values(c6):
    ref, base, excl = c6["ref"], c6["base"], c6["excluded"]
    assert ref["idx"][0] == int(np.argmax(np.where(excl, -np.inf, base)))          # acq_1 = base
    assert ref["val"][0] == base[ref["idx"][0]]
    assert np.all(np.diff(ref["val"]) < 0)                                         # strictly decreasing
    assert len(set(ref["idx"])) == Q and not excl[ref["idx"]].any()
    # the penalty is never positive: conditioning only removes variance
    assert np.all(ref["acq_last"] <= base + 1e-15)
    # replaying the picks reproduces the batch
    again = G.gibbon_reference(c6["x"], c6["y"], c6["pts"], c6["pm"], c6["pv"], c6["ls"], 1e-6, 1e-10, Q, excl, base,
                               picks=ref["idx"])
    assert np.array_equal(again["idx"], ref["idx"]) and np.array_equal(again["var"], ref["var"])


def test_batch_spreads(c6):
    """On the reference alone: the batch's closest pair is farther apart than the farthest pair of
    the top-q of `base` (q neighbours of one maximum)."""
    top = np.argsort(-np.where(c6["excluded"], -np.inf, c6["base"]), kind="stable")[:Q]
    lo, _ = G.pairwise(c6["pts"][c6["ref"]["idx"]])
    _, hi = G.pairwise(c6["pts"][top])
    print("batch: min pairwise distance", lo, "; top-q of base: max pairwise distance", hi)
    assert lo > hi


def test_plugin_form_fails(c6):
    """The documented failure: with the conditioned variance inside g, gamma < 0 for the draws with
    y* < mu, a smaller sigma makes it more negative and g(-inf) = +inf -- the value of a later pick
    RISES next to an earlier one, and the batch is a clump of grid neighbours."""
    idx, val = G.plugin_reference(c6["x"], c6["y"], c6["pts"], c6["pm"], c6["pv"], c6["ls"], 1e-6, 1e-10, Q,
                                  c6["excluded"], c6["mu"], c6["ystar"])
    lo, _ = G.pairwise(c6["pts"][idx])
    print("plug-in picks", idx, "values", val, "min pairwise distance", lo)
    assert lo == 1.0                                                    # grid neighbours
    assert np.any(np.diff(val) > 0)                                     # a later pick is worth MORE
    assert idx[0] == c6["ref"]["idx"][0]                                # the same first pick
    assert G.pairwise(c6["pts"][c6["ref"]["idx"]])[0] > 2.0             # which the penalty form does not do


def test_compose_bound_and_limits():
    base = np.array([0.5, np.nan, 0.25, 1.0, 2.0])
    var0 = np.array([[1.0, 1.0, 0.0, 1.0, np.nan], [2.0, 2.0, 2.0, 2.0, 2.0]])
    var = np.array([[0.5, 0.5, 0.0, np.nan, 1.0], [1.0, 2.0, 1.0, 2.0, 2.0]])
    acq, bound = G.compose(base, var, var0)
    assert acq[0] == 0.5 + 0.5 * (np.log(0.5) + np.log(0.5))
    assert np.isnan(acq[1]) and np.isnan(acq[3]) and np.isnan(acq[4])
    assert acq[2] == 0.25 + 0.5 * np.log(0.5)                           # var0 == 0 contributes nothing
    assert bound[0] == 8 * G.U * (0.5 + 2 * np.log(2.0)) + G.TINY

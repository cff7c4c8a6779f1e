"""numpy reference of the GIBBON batch (bo_select_batch_gibbon, acquisition.select_batch_gibbon) for
tests/test_gibbon_ref.py and tests/test_gpu_gibbon.py.

Independent of the device formulation: the variance after t picks is bucb_ref.posterior(..., extra=
picks), the posterior variance of a GP trained on X u {p_1..p_t} from the inverse of the augmented
Gram matrix (jitter on every point), from scratch at every step -- no recursion, no weight vectors.

    acq_1 = base
    acq_t = base + 0.5 sum_o log(var_o^(t-1) / var_o^0)        (o ascending; var_o^0 == 0 adds 0)
    p_t   = the best available candidate of acq_t (NaN first, descending value, ascending index)

numpy + scipy only: no device, no library.
"""
import numpy as np
from scipy import special

import bucb_ref as R

U = 2.0 ** -53
TINY = 2.0 ** -1022
RTOL = R.RTOL


def log_ratio(var, var0):
    """log(fl(var / var0)) per objective and candidate [n_obj, M]; 0 where var0 == 0."""
    with np.errstate(all="ignore"):
        lg = np.log(var / var0)
    return np.where(var0 == 0.0, 0.0, lg)


def compose(base, var, var0):
    """(acq, bound): fl(base + 0.5 P) with P summed in f64, o ascending, and the bound of the exact
    composition: (n_obj + 6) 2^-53 (|base| + sum_o |log r_o|) + 2^-1022 -- the two logs within 1 ulp
    each, n_obj roundings of the running sum (the terms share a sign, so sum |log r_o| bounds every
    partial sum), one rounding of the final add."""
    lg = log_ratio(var, var0)
    p = np.zeros(lg.shape[1])
    for o in range(lg.shape[0]):
        p = p + lg[o]
    acq = base + 0.5 * p
    with np.errstate(all="ignore"):
        bound = (lg.shape[0] + 6) * U * (np.abs(base) + np.abs(lg).sum(axis=0)) + TINY
    return acq, bound


def margin(acq, bound, var, pv, avail, best):
    """min over the available j != best of (a_best - a_j) - (E_best + E_j) - (B_best + B_j):
    E_j = 0.5 sum_o log1p(10 RTOL pv_o / var_o(j)) is the most a_j can gain, and
    E_best = -0.5 sum_o log1p(-10 RTOL pv_o / var_o(best)) the most a_best can lose, when every
    variance is off by ten times the parity rule RTOL pv_o; B the composition's bound.  Positive:
    any implementation that meets the variance rule and the composition's bound picks `best`.
    var = None: the first pick, taken from `base` itself (E = B = 0)."""
    idx = np.flatnonzero(avail)
    idx = idx[idx != best]
    if idx.size == 0:
        return np.inf
    gap = acq[best] - acq[idx]
    if var is None:
        return float(np.min(gap))
    with np.errstate(all="ignore"):
        rel = 10.0 * RTOL * np.asarray(pv)[:, None] / var
        e_up = 0.5 * np.log1p(rel).sum(axis=0)
        e_dn = -0.5 * np.log1p(-rel).sum(axis=0)          # rel >= 1: inf or NaN, the margin fails
    m = gap - (e_dn[best] + e_up[idx]) - (bound[best] + bound[idx])
    m = np.where(np.isnan(m), -np.inf, m)
    return float(np.min(m))


def gibbon_reference(x, y, cand, pm, pv, ls, jitter, min_var, q, excluded, base, picks=None, var0=None):
    """The batch over `cand` (the shard's points, local indices).  Returns a dict: idx [q] (local,
    -1 = none left), val [q], margins [q] (see margin()), var (after all picks), acq_last (the
    array the last pick was taken from), var0 (the input of the device call).  `picks`: take these
    local indices instead of the arg-max (conditioning on the device's own choice).  `var0`: use
    this array as the unconditioned variance (a NaN planted in it) -- later variances are still the
    posterior's."""
    _, v0 = R.posterior(x, y, cand, pm, pv, ls, jitter, min_var)
    nan0 = None
    if var0 is not None:
        nan0 = np.isnan(var0)
        v0 = var0
    avail = ~np.asarray(excluded, dtype=bool)
    base = np.asarray(base, dtype=np.float64)
    var = v0
    idx, val, margins = [], [], []
    acq = base
    for t in range(q):
        if t == 0:
            acq, bound, mv = base, None, None
        else:
            acq, bound = compose(base, var, v0)
            mv = var
        p, _ = R.best(acq, avail)
        margins.append(margin(acq, bound, mv, pv, avail, p) if p >= 0 and not np.isnan(acq[p]) else np.inf)
        if picks is not None:
            p = int(picks[t])
        idx.append(p)
        val.append(acq[p] if p >= 0 else -np.inf)
        if p >= 0:
            avail[p] = False
            chosen = cand[[i for i in idx if i >= 0]]
            _, var = R.posterior(x, y, cand, pm, pv, ls, jitter, min_var, extra=chosen)
            if nan0 is not None:
                var = np.where(nan0, np.nan, var)
    return {"idx": np.array(idx), "val": np.array(val), "margins": np.array(margins), "var": var,
            "acq_last": acq, "var0": v0}


# ------------------------------------------------------------------ the max-value entropy as `base`
def g_f64(x):
    """g(x) = x phi(x) / (2 Phi(x)) - ln Phi(x) in f64, the three branches of include/bo_amd.h."""
    x = np.asarray(x, dtype=np.float64)
    out = np.full(x.shape, np.nan)
    with np.errstate(all="ignore"):
        p = x >= 0
        xp = x[p]
        q = 0.5 * special.erfc(xp * 0.7071067811865476)
        ph = np.exp(-0.5 * xp * xp) * 0.3989422804014327
        out[p] = np.where(ph == 0.0, 0.0, xp * ph) / (2.0 * (1.0 - q)) - np.log1p(-q)
        a = x <= -2.0 ** 27
        out[a] = np.log(-x[a]) + 0.4189385332046727
        m = (x < 0) & ~a
        t = -x[m] * 0.7071067811865476
        e = special.erfcx(t)
        out[m] = t * t - t / (1.772453850905516 * e) - np.log(0.5 * e)
    return out


def posterior_mean_cov(x, y, pts, pm, pv, ls, jitter):
    """mu [n_obj, M] (objective units) and the posterior covariance [n_obj, M, M] of the GP on x."""
    n_obj = len(pv)
    mu = np.empty((n_obj, pts.shape[0]))
    cov = np.empty((n_obj, pts.shape[0], pts.shape[0]))
    for o in range(n_obj):
        ks = R.rbf(pts, x, pv[o], ls[o])
        kinv = np.linalg.inv(R.rbf(x, x, pv[o], ls[o]) + jitter * np.eye(x.shape[0]))
        mu[o] = pm[o] + ks @ (kinv @ (y[:, o] - pm[o]))
        cov[o] = R.rbf(pts, pts, pv[o], ls[o]) - ks @ kinv @ ks.T
    return mu, cov


def sampled_maxima(mu, cov, n_s, seed):
    """ystar [n_s, n_obj]: the maxima over all points of exact joint posterior draws."""
    rng = np.random.default_rng(seed)
    n_obj, m = mu.shape
    ystar = np.empty((n_s, n_obj))
    for o in range(n_obj):
        w, v = np.linalg.eigh(cov[o])
        root = v * np.sqrt(np.maximum(w, 0.0))
        f = mu[o][None, :] + rng.standard_normal((n_s, m)) @ root.T
        ystar[:, o] = f.max(axis=1)
    return ystar


def mes(mu, var, ystar):
    """acq [M] = (1/S) sum_s sum_k g((y*_sk - mu_k) / sqrt(|var_k|))."""
    with np.errstate(all="ignore"):
        gam = (ystar[:, :, None] - mu[None]) / np.sqrt(np.abs(var))[None]
    return g_f64(gam).sum(axis=(0, 1)) / ystar.shape[0]


def plugin_reference(x, y, cand, pm, pv, ls, jitter, min_var, q, excluded, mu, ystar):
    """The form that does NOT work, kept as the documented failure: the conditioned variance put
    into the max-value entropy itself.  Returns (idx [q], val [q])."""
    _, var = R.posterior(x, y, cand, pm, pv, ls, jitter, min_var)
    avail = ~np.asarray(excluded, dtype=bool)
    idx, val = [], []
    for t in range(q):
        acq = mes(mu, var, ystar)
        p, _ = R.best(acq, avail)
        idx.append(p)
        val.append(acq[p])
        avail[p] = False
        _, var = R.posterior(x, y, cand, pm, pv, ls, jitter, min_var, extra=cand[idx])
    return np.array(idx), np.array(val)


def pairwise(points):
    """(min, max) pairwise distance of the rows of `points`."""
    d = np.sqrt(((points[:, None, :] - points[None, :, :]) ** 2).sum(-1))
    iu = np.triu_indices(points.shape[0], 1)
    return float(d[iu].min()), float(d[iu].max())

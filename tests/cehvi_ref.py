"""The feasibility-weighted EHVI in numpy (outcome constraints; include/bo_amd.h,
bo_constrained_ehvi): the probability of feasibility in its tail-safe form and its product with the
closed form of tests/ehvi_ref.py.  PARITY UNPINNED by the reference, which has neither.
tests/test_cehvi.py pins `pof` against mpmath at 60 digits and `cehvi` against a Monte-Carlo mean.

    P_j = P(lo_j <= Y_j <= hi_j),  Y_j ~ N(mu_j, sigma_j^2);   cehvi = EHVI(objective rows) prod_j P_j
"""
import numpy as np
from scipy.special import erfc

import ehvi_ref as R

U = 2.0 ** -53


def tail(z):
    """Q(z) = 1 - Phi(z) = erfc(z / sqrt 2) / 2."""
    return 0.5 * erfc(np.asarray(z, dtype=np.float64) / np.sqrt(2.0))


def pof_terms(mu, sigma, lo, hi):
    """(P, T, z): P(lo <= Y <= hi) as a difference of positive tail terms,
         za > 0:  Q(za) - Q(zb)      zb < 0:  Q(-zb) - Q(-za)      else:  1 - Q(zb) - Q(-za)
    with za = (lo - mu) / sigma, zb = (hi - mu) / sigma; T the larger of the two positive terms (1
    in the central branch) and z that term's argument (0 in the central branch): what the error
    bound (8 z^2 + 32) u T is stated in.  sigma = 0: 1 inside [lo, hi], else 0 (T = 1, z = 0); NaN in
    mu or sigma gives NaN.  Arrays broadcast."""
    mu, sigma, lo, hi = np.broadcast_arrays(*(np.asarray(a, dtype=np.float64) for a in (mu, sigma, lo, hi)))
    with np.errstate(divide="ignore", invalid="ignore"):
        za = (lo - mu) / sigma
        zb = (hi - mu) / sigma
    above = za > 0
    below = ~above & (zb < 0)
    t1 = np.where(above, za, np.where(below, -zb, zb))
    t2 = np.where(above, zb, -za)
    q1, q2 = tail(t1), tail(t2)
    tails = above | below
    p = np.where(tails, q1, 1.0 - q1) - q2
    big = np.where(tails, q1, 1.0)                      # t1 <= t2 in the tail branches: q1 is the larger
    z = np.where(tails, t1, 0.0)
    zero = sigma == 0.0
    p = np.where(zero, ((lo <= mu) & (mu <= hi)).astype(np.float64), p)
    big = np.where(zero, 1.0, big)
    z = np.where(zero, 0.0, z)
    nan = np.isnan(mu) | np.isnan(sigma)
    return np.where(nan, np.nan, p), np.where(nan, np.nan, big), np.where(nan, np.nan, z)


def pof(mu, sigma, lo, hi):
    return pof_terms(mu, sigma, lo, hi)[0]


def pof_bound(mu, sigma, lo, hi):
    """(8 z^2 + 32) u T: the absolute error allowed to one evaluation of pof."""
    _, big, z = pof_terms(mu, sigma, lo, hi)
    return (8.0 * z * z + 32.0) * U * big


def pof_product(mu_con, var_con, bounds):
    """prod_j P_j, left to right, from the constraint rows [n_con, n] and bounds [n_con, 2]; 1 without
    constraints.  sigma = sqrt(|var|)."""
    mu_con = np.asarray(mu_con, dtype=np.float64)
    sigma = np.sqrt(np.abs(np.asarray(var_con, dtype=np.float64)))
    p = np.ones(mu_con.shape[1])
    for j, (lo, hi) in enumerate(np.asarray(bounds, dtype=np.float64).reshape(-1, 2)):
        pj = pof(mu_con[j], sigma[j], lo, hi)
        p = pj if j == 0 else p * pj
    return p


def cehvi(mu, var, boxes, bounds):
    """mu, var: [n_obj + n_con, n], the objective rows first; boxes: hypervolume_boxes' output for the
    FEASIBLE front, [n_boxes, 2 n_obj]; bounds: [n_con, 2].  NaN in any row gives NaN.  Returns [n]."""
    mu = np.asarray(mu, dtype=np.float64)
    var = np.asarray(var, dtype=np.float64)
    bounds = np.asarray(bounds, dtype=np.float64).reshape(-1, 2)
    m = mu.shape[0] - bounds.shape[0]
    return R.ehvi(mu[:m], var[:m], boxes) * pof_product(mu[m:], var[m:], bounds)


def feasible(y, n_obj, bounds):
    """Rows of y ([n, n_obj + n_con]) whose constraint outputs lie inside their bounds."""
    y = np.asarray(y, dtype=np.float64)
    b = np.asarray(bounds, dtype=np.float64).reshape(-1, 2)
    g = y[:, n_obj:]
    return np.all((g >= b[:, 0]) & (g <= b[:, 1]), axis=1)

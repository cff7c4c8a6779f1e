"""Independent statement of the max-value entropy search acquisition (acquisition "mes";
include/bo_amd.h states the quantity), in mpmath, with the f64 restatement of the device's
three-branch g and the rounding rule's bound.  numpy + scipy + mpmath only: no device, no library.

    g(x)   = x phi(x) / (2 Phi(x)) - ln Phi(x)
    acq(c) = (1/S) sum_s sum_k g((y*_sk - mu_k(c)) / sqrt(|var_k(c)|))
    rule:    |acq_dev - acq_ref| <= u/S sum_sk [C (1 + gamma_sk^2 / 2) + S n_obj] g_ref(gamma_sk) + 2^-1022,
             u = 2^-53, C = 32 for the device, 16 for the f64 restatement on the CPU
"""
import numpy as np
import mpmath as mp
from scipy import special

U = 2.0 ** -53
TINY = 2.0 ** -1022
DPS = 60                  # g cancels x^2 / 2 <= 5e15 against itself at x = -1e8: 16 digits lost of 60
CUT = -2.0 ** 27          # at or below: the asymptote
C_DEVICE = 32.0
C_F64 = 16.0


def g_mp(x):
    """g at x (a float, or an mpf) as an mpf at DPS digits; g(+inf) = 0, g(-inf) = +inf, g(NaN) = NaN."""
    with mp.workdps(DPS):
        x = mp.mpf(x)
        if mp.isnan(x):
            return mp.nan
        if x == mp.inf:
            return mp.mpf(0)
        if x == -mp.inf:
            return mp.inf
        phi = mp.exp(-x * x / 2) / mp.sqrt(2 * mp.pi)
        if x >= 0:
            q = mp.erfc(x / mp.sqrt(2)) / 2                  # 1 - Phi, positive to full relative accuracy
            return x * phi / (2 * (1 - q)) - mp.log1p(-q)
        cdf = mp.erfc(-x / mp.sqrt(2)) / 2
        return x * phi / (2 * cdf) - mp.log(cdf)


def entropy_difference_mp(x):
    """H[N(0, 1)] - H[N(0, 1) truncated above at x] by quadrature: what g is defined as."""
    with mp.workdps(30):
        x = mp.mpf(x)
        cdf = mp.ncdf(x)

        def integrand(y):
            p = mp.npdf(y) / cdf
            return -p * mp.log(p) if p > 0 else mp.mpf(0)
        lo = min(x - 1, mp.mpf(-40))
        pts = [lo] + [t for t in (-20, -10, -5, -2, 0, 2, 5) if lo < t < x] + [x]
        h_trunc = mp.quad(integrand, pts)
        return mp.log(2 * mp.pi * mp.e) / 2 - h_trunc


def g_f64(x):
    """The device's three branches restated in f64 (numpy, scipy's erfc / erfcx); x: array."""
    x = np.asarray(x, dtype=np.float64)
    out = np.full(x.shape, np.nan)
    with np.errstate(all="ignore"):
        p = x >= 0
        xp = x[p]
        q = 0.5 * special.erfc(xp * 0.7071067811865476)
        ph = np.exp(-0.5 * xp * xp) * 0.3989422804014327
        xph = np.where(ph == 0.0, 0.0, xp * ph)             # x = +inf: inf * 0
        out[p] = xph / (2.0 * (1.0 - q)) - np.log1p(-q)
        a = x <= CUT
        out[a] = np.log(-x[a]) + 0.4189385332046727
        m = (x < 0) & (x > CUT)
        t = -x[m] * 0.7071067811865476
        e = special.erfcx(t)
        out[m] = t * t - t / (1.772453850905516 * e) - np.log(0.5 * e)
    return out


def unit(x, g):
    """u (1 + x^2 / 2) g: the rounding rule's unit at x (0 where g = 0, also at x = +inf)."""
    x = np.asarray(x, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(g == 0.0, 0.0, U * (1.0 + 0.5 * x * x) * g)


def gamma_mp(ystar, mu, var):
    """(kind, gamma): gamma = (y* - mu) / sqrt(|var|) from the f64 inputs, unrounded; kind names the
    limits: 'nan', 'zero' (g = 0), 'inf' (g = +inf) or 'g' (evaluate g at gamma)."""
    if np.isnan(ystar) or np.isnan(mu) or np.isnan(var):
        return "nan", None
    if var == 0.0:
        d = ystar - mu                                  # only its sign matters
        if np.isnan(d):
            return "nan", None
        return ("zero" if d >= 0 else "inf"), None
    if ystar == np.inf:
        return "zero", None
    if ystar == -np.inf:
        return "inf", None
    with mp.workdps(DPS):
        return "g", (mp.mpf(float(ystar)) - mp.mpf(float(mu))) / mp.sqrt(abs(mp.mpf(float(var))))


def acquisition_ref(mu, var, ystar, c=C_DEVICE):
    """(acq_ref [n] as f64, bound [n]) of the rule, from f64 mu / var [n_obj, n] and ystar [S, n_obj].
    Where acq_ref is not finite (NaN or +inf: the limits) the bound is 0: the device must give that value."""
    mu = np.asarray(mu, dtype=np.float64)
    var = np.asarray(var, dtype=np.float64)
    ystar = np.asarray(ystar, dtype=np.float64)
    n_obj, n = mu.shape
    n_s = ystar.shape[0]
    assert var.shape == mu.shape and ystar.shape == (n_s, n_obj)
    acq = np.empty(n)
    bound = np.empty(n)
    with mp.workdps(DPS):
        for i in range(n):
            tot, bnd, special_value = mp.mpf(0), mp.mpf(0), None
            for s in range(n_s):
                for k in range(n_obj):
                    kind, gam = gamma_mp(ystar[s, k], mu[k, i], var[k, i])
                    if kind == "nan":
                        special_value = np.nan
                    elif kind == "inf":
                        if special_value is None:
                            special_value = np.inf
                    elif kind == "g":
                        g = g_mp(gam)
                        if g == mp.inf:                        # gamma = -inf (an infinite mu)
                            if special_value is None:
                                special_value = np.inf
                        elif g != 0:                           # g = 0 (gamma = +inf) adds nothing
                            tot += g
                            bnd += (c * (1 + gam * gam / 2) + n_s * n_obj) * g
            if special_value is not None:
                acq[i], bound[i] = special_value, 0.0
            else:
                acq[i] = float(tot / n_s)
                bound[i] = float(mp.mpf(U) / n_s * bnd) + TINY
    return acq, bound


def check_rule(acq_dev, acq_ref, bound):
    """The share of candidates that miss the rule, and the worst |error| / bound."""
    acq_dev = np.asarray(acq_dev, dtype=np.float64)
    fin = np.isfinite(acq_ref)
    same = np.where(np.isnan(acq_ref), np.isnan(acq_dev), acq_dev == acq_ref)
    with np.errstate(all="ignore"):
        err = np.abs(acq_dev - acq_ref)
        ok = np.where(fin, err <= bound, same)
        ratio = np.where(fin, err / bound, 0.0)
    return 1.0 - ok.mean(), float(ratio.max()) if ratio.size else 0.0


def fma_once(scale, m, shift):
    """fl(shift + scale * m), one rounding (the maxima's map), NaN / inf as IEEE."""
    if np.isnan(m):
        return np.nan
    if np.isinf(m):
        return float(m) if scale > 0 else float(-m)
    with mp.workdps(DPS):
        return float(mp.mpf(float(scale)) * mp.mpf(float(m)) + mp.mpf(float(shift)))


def maxima_ref(paths, shift, scale):
    """ystar [rows] of bo_path_maxima for paths [rows, n_cand] (row r: objective r mod n_obj): NaN
    ignored, all-NaN or empty -> NaN, a zero maximum counts as +0."""
    n_obj = len(shift)
    out = np.empty(paths.shape[0])
    for r, row in enumerate(paths):
        fin = row[~np.isnan(row)]
        m = np.nan if fin.size == 0 else float(fin.max()) + 0.0
        out[r] = fma_once(scale[r % n_obj], m, shift[r % n_obj])
    return out


def select_top(acq, excluded, q):
    """The q best non-excluded candidates of acq (no NaN; descending value, ties by ascending index), and
    per pick the gap to the next value in that order (the last pick's: to the best unpicked one)."""
    v = np.where(excluded, -np.inf, np.asarray(acq, dtype=np.float64))
    order = np.argsort(-v, kind="stable")
    picks = order[:q]
    gaps = v[order[:q]] - v[order[1:q + 1]]
    return picks, gaps, order[1:q + 1]

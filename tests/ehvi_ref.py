"""Expected hypervolume improvement in numpy: the closed form per box, written from the textbook
statement and independently of the device's rearrangement of psi (bo_ehvi.hip), plus the Python
mirror of the table form's admission rule (include/bo_amd.h).  PARITY UNPINNED by the reference,
which has no EHVI; tests/test_ehvi.py pins this file against a Monte-Carlo mean of the box sum
that tests/test_hvi.py pins against the brute-force hypervolume.
The exact reference (mpmath, and the rounding rule the device is held to) is tests/ehvi_exact_ref.py.

    EHVI = sum_b prod_k [psi_k(l_bk) - psi_k(u_bk)],   psi_k(a) = E[(Y_k - a)+],  Y_k ~ N(mu_k, sigma_k^2)
"""
import numpy as np
from scipy.special import erfc

HVI_RTOL = 1e-9              # tests/test_hvi.py's margin for this box sum
LDS_BYTES = 160 * 1024       # bo_ehvi.hip: kEhviLdsBytes
TABLE_THREADS = (256, 128, 64)


def psi(mu, sigma, a):
    """E[(Y - a)+] = sigma (phi(z) + z Phi(z)), z = (mu - a) / sigma; max(mu - a, 0) at sigma = 0;
    0 at a = +inf.  mu, sigma: arrays; a: scalar."""
    mu = np.asarray(mu, dtype=np.float64)
    sigma = np.asarray(sigma, dtype=np.float64)
    if np.isposinf(a):
        return np.where(np.isnan(mu) | np.isnan(sigma), np.nan, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = (mu - a) / sigma
        pdf = np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi)
        cdf = 0.5 * erfc(-z / np.sqrt(2.0))
        val = sigma * (pdf + z * cdf)
    return np.where(sigma == 0.0, np.maximum(mu - a, 0.0), val)


def ehvi(mu, var, boxes):
    """mu, var: [n_obj, n]; boxes: hypervolume_boxes' output [n_boxes, 2 n_obj].  sigma = sqrt(|var|)
    (the UCB's convention).  NaN in any mu_k or var_k gives NaN.  Returns [n]."""
    mu = np.asarray(mu, dtype=np.float64)
    sigma = np.sqrt(np.abs(np.asarray(var, dtype=np.float64)))
    m, n = mu.shape
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 2 * m)
    cache = {}

    def p(k, a):
        if (k, a) not in cache:
            cache[(k, a)] = psi(mu[k], sigma[k], a)
        return cache[(k, a)]

    out = np.zeros(n)
    for b in boxes:
        term = np.ones(n)
        for k in range(m):
            term = term * (p(k, b[k]) - p(k, b[m + k]))
        out += term
    out[np.isnan(mu).any(axis=0) | np.isnan(sigma).any(axis=0)] = np.nan
    return out


def scale(mu, var, reference_point):
    """prod_k psi_k(r_k) + 1: the EHVI over an empty front, an upper bound of every term of the
    box sum, plus one -- what HVI_RTOL multiplies."""
    mu = np.asarray(mu, dtype=np.float64)
    sigma = np.sqrt(np.abs(np.asarray(var, dtype=np.float64)))
    s = np.ones(mu.shape[1])
    for k in range(mu.shape[0]):
        s = s * psi(mu[k], sigma[k], float(reference_point[k]))
    return s + 1.0


def edge_counts(boxes, n_obj):
    """E_k: the number of distinct finite bounds of objective k over the boxes."""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 2 * n_obj)
    out = []
    for k in range(n_obj):
        v = np.concatenate([b[:, k], b[:, n_obj + k]])
        out.append(int(np.unique(v[np.isfinite(v)]).size))
    return out


def table_threads(sum_edges):
    """Mirror of bo_ehvi_table_threads: the table holds sum_edges doubles per thread; the workgroup
    is the largest T of TABLE_THREADS whose table fits the LDS of a CU; 0 when none does."""
    for t in TABLE_THREADS:
        if 8 * sum_edges * t <= LDS_BYTES:
            return t
    return 0

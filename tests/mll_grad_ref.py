"""Extended-precision reference of the MLL's gradient in log(length scale), its f64 numpy restatement and
the scale of its rounding error.  Helper module: no tests in it (tests/test_mll_grad_ref.py,
tests/test_gpu_mll_grad.py).  Problems, LD and U are tests/exact_fit_ref.py's.

The quantity.  Per objective, with exact_fit_ref's notation (a_ij = r2_ij / (2 l^2), E = exp(-a),
C = E + jitter I, r = y - pm, s the population std of r about its own mean, left 1 when it is 0):
    yc = r / s      alpha = C^-1 yc      D_ij = dC_ij / d log l = E_ij r2_ij / l^2 = 2 a_ij E_ij
    g = d MLL / d log l = 1/2 sum_ij (alpha_i alpha_j - C^-1_ij) D_ij
(1/2 alpha^T D alpha from the data-fit term -1/2 yc^T C^-1 yc, -1/2 tr(C^-1 D) from -1/2 log det C).  pv does
not enter: d MLL / d pv = 0 exactly.  At N = 1 the only r2 is 0, so g = 0 exactly.

The reference (exact_grad) runs exact_fit_ref's chain in numpy.longdouble: the column Cholesky of C, L^-1 by
forward substitution, C^-1 = L^-T L^-1, and the formula.  Its own error is first order in 2^-64 with the same
amplification as the f64 error below: 2^-11 of an f64 chain's, i.e. below 0.1 in the units err / (u S) whenever
the f64 ratio is below 200.

The restatement (restated_grad) is the chain in f64 numpy with LAPACK's inverse: the Gram, np.linalg.inv, one
Newton step X + X (I - C X), alpha = X yc, the same formula.  It is the oracle whose error defines R.  (The
device takes C^-1 from its augmented Cholesky and leaves the Newton step out: that inverse is the exact inverse
of ONE symmetric C + dC, the picture S_p below is derived in, and measured 0.45 u S at worst where the same
inverse after the Newton step measured 833 u S -- the step makes every column's residual small with a dC of
its own per column and adds rounding of the order u |X|^2 to X.  The restatement, a solve-based inverse with the
step, sits at 0.007..250 u S.)

The scale, first order in u = 2^-53:
    S_g = 1/2 sum_ij (|alpha_i| |alpha_j| + |C^-1_ij|) D_ij
      a relative error of a few u in every term of the sum, in D_ij (exp, r2, the division) and in the
      products, and the summation's own rounding;
    S_p = 1/2 (1 + jitter) (sum_ij |C^-1 D C^-1|_ij + 2 |C^-1 D alpha|_1 |alpha|_1)
      the computed inverse is the exact inverse of C + dC with |dC_ij| <= c u (1 + jitter) (a Cholesky-based
      inverse; exact_fit_ref's S_chol argument): d(C^-1) = -C^-1 dC C^-1 changes
      -1/2 tr(C^-1 D) by 1/2 tr(C^-1 dC C^-1 D) = 1/2 sum_ij dC_ij (C^-1 D C^-1)_ji, and alpha by
      -C^-1 dC alpha, which changes 1/2 alpha^T D alpha by -(C^-1 D alpha)^T dC alpha, at most
      c u (1 + jitter) |C^-1 D alpha|_1 |alpha|_1;
    S = S_g + S_p.
|C^-1| and alpha for S come from an f64 inverse (a scale needs one digit).  ratio = err / (u S); 0 / 0 (N = 1:
every D_ij is 0) counts as 0.

grad_R is the restatement's largest ratio over GRAD_CASES; the device is held to 8 R (DESIGN section 5's rule).
"""

import numpy as np

import exact_fit_ref as F
from exact_ref import LD, LD_OK, U, split_ld

TIGHT = F.TIGHT
VALUE_NS = (1, 2, 31, 32, 33, 64, 65, 257, 513)
VALUE_CASES = [(n, 1e-8, "") for n in VALUE_NS]
GRAD_CASES = VALUE_CASES + [(100, 1e-4, ""), (33, 1e-8, "std0"), (33, 1e-8, "pm")]
_CACHE = {}


def _std_scale(r):
    s2 = np.mean((r - np.mean(r)) ** 2)
    return np.sqrt(s2) if s2 > 0 else type(s2)(1)


def _chain_ld(x, y_o, pm_o, ls_o, jitter):
    """(mll, g, alpha, Cinv) in long double; None on a non-positive pivot."""
    if not LD_OK:
        raise RuntimeError("the gradient's reference needs a long double wider than f64")
    n = x.shape[0]
    xl = np.asarray(x, dtype=np.float64).astype(LD)
    d = xl[:, None, :] - xl[None, :, :]
    r2 = np.einsum("ijd,ijd->ij", d, d)
    ls = LD(float(ls_o))
    E = np.exp(-(r2 / (2 * ls * ls)))
    A = E.copy()
    A[np.diag_indices(n)] += LD(float(jitter))
    r = np.asarray(y_o, dtype=np.float64).astype(LD) - LD(float(pm_o))
    yc = r / _std_scale(r)
    L = A.copy()
    for j in range(n):
        if not L[j, j] > 0:
            return None
        dj = np.sqrt(L[j, j])
        L[j, j] = dj
        if j + 1 < n:
            L[j + 1:, j] /= dj
            col = L[j + 1:, j].copy()
            L[j + 1:, j + 1:] -= np.outer(col, col)
    L = np.tril(L)
    Li = np.zeros((n, n), dtype=LD)                     # L Li = I, row by row
    for i in range(n):
        row = -(L[i, :i] @ Li[:i, :]) if i else np.zeros(n, dtype=LD)
        row[i] += 1
        Li[i, :] = row / L[i, i]
    Cinv = Li.T @ Li
    alpha = Cinv @ yc
    D = E * r2 / (ls * ls)
    g = (np.sum((np.outer(alpha, alpha) - Cinv) * D)) / 2
    z = Li @ yc
    mll = -np.sum(z * z) / 2 - np.sum(np.log(np.diag(L))) - LD(n) / 2 * F.LOG_2PI
    return mll, g, alpha, Cinv


def mll_ld(x, y_o, pm_o, ls_o, jitter):
    """exact_fit_ref's MLL term as an unrounded long double (for the central difference)."""
    return F._mll_ld(x, y_o, pm_o, ls_o, jitter)[0]


def exact_grad(x, y_o, pm_o, ls_o, jitter):
    """The reference gradient of one objective and its scale: dict with g (rounded to f64), hi, lo (the
    unrounded value as two f64), mll (f64, the chain's own value), S_g, S_p, S, n."""
    x = np.asarray(x, dtype=np.float64)
    y_o = np.asarray(y_o, dtype=np.float64)
    n = x.shape[0]
    res = _chain_ld(x, y_o, pm_o, ls_o, jitter)
    assert res is not None, "a non-positive pivot: a wrongly chosen case"
    mll, g, _, _ = res
    hi, lo = (float(v) for v in split_ld(g))
    # the scale, in f64
    d = x[:, None, :] - x[None, :, :]
    r2 = np.einsum("ijd,ijd->ij", d, d)
    ls2 = float(ls_o) ** 2
    E = np.exp(-r2 / (2.0 * ls2))
    D = E * r2 / ls2
    Ci = np.linalg.inv(E + float(jitter) * np.eye(n))
    r = y_o - float(pm_o)
    al = Ci @ (r / _std_scale(r))
    aal = np.abs(al)
    S_g = 0.5 * float(aal @ D @ aal + (np.abs(Ci) * D).sum())
    S_p = 0.5 * (1.0 + float(jitter)) * float(np.abs(Ci @ D @ Ci).sum() + 2.0 * np.abs(Ci @ D @ al).sum() * aal.sum())
    return dict(g=hi, hi=hi, lo=lo, mll=float(mll), S_g=S_g, S_p=S_p, S=S_g + S_p, n=n)


def restated_grad(x, y_o, pm_o, ls_o, jitter):
    """The chain in f64 numpy: np.linalg.inv, one Newton step, the formula (the oracle behind R)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    d = x[:, None, :] - x[None, :, :]
    r2 = np.einsum("ijd,ijd->ij", d, d)
    ls2 = float(ls_o) * float(ls_o)
    E = np.exp(-0.5 * r2 / ls2)
    Cm = E + float(jitter) * np.eye(n)
    X0 = np.linalg.inv(Cm)
    X = X0 + X0 @ (np.eye(n) - Cm @ X0)
    r = np.asarray(y_o, dtype=np.float64) - float(pm_o)
    al = X @ (r / _std_scale(r))
    return float(0.5 * np.sum((np.outer(al, al) - X) * (E * (r2 / ls2))))


def grad_error(got, ref):
    return float(abs((LD(float(got)) - LD(ref["hi"])) - LD(ref["lo"])))


def grad_ratio(got, ref):
    err = grad_error(got, ref)
    return 0.0 if err == 0.0 else err / (U * ref["S"])


def grad_case(key):
    """exact_fit_ref.mll_problem(key) with the three objectives' references and restated gradients, once."""
    if key not in _CACHE:
        p = F.mll_problem(key)
        refs = [exact_grad(p["x"], p["y"][:, o], p["pm"][o], p["ls"][o], p["jitter"]) for o in range(3)]
        rest = [restated_grad(p["x"], p["y"][:, o], p["pm"][o], p["ls"][o], p["jitter"]) for o in range(3)]
        _CACHE[key] = dict(p, grefs=refs, restated=rest)
    return _CACHE[key]


def grad_R():
    """The restatement's largest err / (u S) over GRAD_CASES."""
    if "R" not in _CACHE:
        _CACHE["R"] = max(grad_ratio(c["restated"][o], c["grefs"][o]) for c in map(grad_case, GRAD_CASES)
                          for o in range(3))
    return _CACHE["R"]


# ---- the numpy fit: the restatement under scipy's L-BFGS-B and Powell (the choice of the GPU fit test's problems)

def numpy_value_grad(x, y, pm, ls, jitter=1e-8):
    """(sum of the MLL terms, gradient in log ls [n_obj]) in f64 numpy, LAPACK's Cholesky."""
    from scipy.linalg import cho_factor, cho_solve
    n, n_obj = x.shape[0], len(ls)
    d = x[:, None, :] - x[None, :, :]
    r2 = np.einsum("ijd,ijd->ij", d, d)
    tot, g = 0.0, np.zeros(n_obj)
    for o in range(n_obj):
        ls2 = float(ls[o]) ** 2
        E = np.exp(-0.5 * r2 / ls2)
        cf = cho_factor(E + jitter * np.eye(n), lower=True)
        r = y[:, o] - pm[o]
        yc = r / _std_scale(r)
        Ci = cho_solve(cf, np.eye(n))
        al = Ci @ yc
        tot += -0.5 * float(yc @ al) - float(np.log(np.diag(cf[0])).sum()) - 0.5 * n * np.log(2 * np.pi)
        g[o] = 0.5 * float(np.sum((np.outer(al, al) - Ci) * (E * (r2 / ls2))))
    return tot, g

"""Extended-precision references of the fit path -- compute_mll's per-objective term and invert_k's
backward error -- and rounding-error bounds that hold at any cond(K).  Helper module: no tests in it
(tests/test_exact_fit_ref.py, tests/test_gpu_fit_exact.py).  U, LD, LD_OK, split_ld are tests/exact_ref.py's.

The MLL's reference.  Per objective, in numpy.longdouble (64-bit significand; mpmath at 128 bits where
the platform's long double is no wider than f64 -- there a Cholesky costs N^3 / 3 mpmath operations, and
the sampled columns of the residual are thinned by exact_ref.SUBSAMPLE):
    a_ij = |x_i - x_j|^2 / (2 l^2)    E_ij = exp(-a_ij)    A = E + jitter I    r = y - pm
    s^2 = the population variance of r about its own mean (np.std, oracle_np.py:90-92); D is left
          unscaled when it is 0 (bo_fit.hip:1838)
    L = chol(A)    z = L^-1 r    w = L^-T z    D = |z|^2 / s^2    Lam = 2 sum log L_ii
    mll = -D / 2 - Lam / 2 - (N / 2) log 2 pi
from the f64 inputs exactly as given.  pv does not enter: the device factors the correlation matrix
(bo_fit.hip:249-252).  A non-positive pivot makes the value NaN.

The MLL's bound, first order in u = 2^-53.  A Cholesky whose entries each pass through at most c
roundings computes the exact factor of A + dA with |dA_ij| <= c u (|L| |L|^T)_ij <= c u sqrt(A_ii A_jj)
= c u (1 + jitter), and the bordered row z that of r + dr with |dr_j| <= c u |z|_2 sqrt(A_jj),
|z|_2^2 = w^T A w <= (1 + jitter) |w|_1^2.  So  dD = (-w^T dA w + 2 w . dr) / s^2  and
dLam = tr(A^-1 dA)  are bounded by 3c u and c u times the two halves of
    S_chol = (1 + jitter) (|w|_1^2 / s^2 + sum_ij |A^-1|_ij) / 2.
The Gram entries' own rounding is a relative error (c1 + c2 a_ij) u in E_ij (c1: exp and, on the
diagonal, the addition of the jitter; c2: the exponent's argument), the same dD and dLam with dA = that:
    S_gram = (sum_ij |w_i| (1 + a_ij) E_ij |w_j| / s^2 + sum_ij |A^-1_ij| (1 + a_ij) E_ij) / 2.
What is left is relative to the terms themselves and to r:
    S_fix  = |D| / 2 + |Lam| / 2 + (N / 2) log 2 pi + |mll| + sum_i |w_i| (|y_i| + |pm|) / s^2
(r = y - pm, one rounding of at most u (|y_i| + |pm|) in r_i; |Lam| stands for sum |2 log L_ii|: with a
unit diagonal L_ii <= sqrt(1 + jitter), so the logarithms share their sign up to N jitter).
    tol_hard = u (C_chol S_chol + C_gram S_gram + C_fix S_fix).
|A^-1| comes from an f64 inverse (a scale needs one digit).  First order suffices while
C_chol u cond(A) < 0.1 (cond(A) <= N / jitter): the second-order terms are that fraction of the bound.
check_mll asserts it, so that a case outside it is a wrongly chosen case, not a pass.

The constants, counted from bayesopt_smart_amd/csrc/bo_fit.hip (n_p = 32 ceil(N / 32), nbt = n_p / 32;
the persistent and the launch-per-step schedule run the same roles, so one count serves both):
  c, the roundings one product l_ik l_jk passes on its way into an entry of L or z:
    its own trailing update: 32 FMAs of a rank-32 step from a zero accumulator (update_role, :599-603;
      panel_role :453-456), 64 where the MLL's even launches apply two steps at once (UPD 2, :570);
      no update at all when n_p = 32                                              min(64, n_p - 32)
    the subtraction A - D that ends every update, its own and each later step's (:613, :465)    nbt
    the panel sweep, at most 31 FMAs inside the 32 x 32 tile (:506, :518)                         31
    the pivot: rsqrt_sqrt (:127-139) is v_rsq_f64 (2^-29) and two coupled Goldschmidt steps, no
      division.  The first step leaves g and h with one rounding each on top of (3/2) 2^-58; the
      second cannot remove those (g' = g (1 + r) with r = -(e_g + e_h) / 2 leaves (e_g - e_h) / 2)
      and adds its own: at most 3 ulp in sqrt and in 1 / sqrt.  L_ij = a_ij rs: 3 + 1 = 4; the
      diagonal enters squared: 6; the larger with one of slack                                     7
    c = min(64, n_p - 32) + nbt + 38,     C_chol = 3 c    (dA once, dr twice).
  C_gram = dim + 4: fit_init_kernel (:332-337) rounds each difference (2 in its square), runs dim FMAs,
    the host squares l (:1805) and the kernel divides: dim + 4 on a_ij; exp 1 and jitter 1 stay below.
  C_fix = nbt + ceil(N / 256) + 56: |z|^2 in 32 FMAs per step (:546) and nbt host additions (:1833-1836)
    32 + nbt; the variance (:283-299) one subtraction, one 256-way strided sum and an 8-level tree
    twice, the mean, a square and a division: ceil(N / 256) + 13; the division by it 1; log (1 ulp), the
    6-level wave sum (:535-537) and nbt host additions of Lam, the three products and two additions of
    the output (:1839): within the 10 left.
  The LAPACK oracle and the numpy restatement (path "oracle"): c = N + 7 (unblocked), C_gram = dim + 6
    ((pv e) / pv), C_fix = N + 16.
No MLL constant may exceed 3 n_p + 64; fit_constants asserts it.

The inverse's reference is a residual.  With K the f64 array handed to the device, used as data,
A = K + jitter I and X the computed inverse, per sampled column j in long double
    rho_j = |A X[:, j] - e_j|_inf / (u alpha |X[:, j]|_1),       alpha = max_i (K_ii + jitter):
a row of the product is a pairwise sum of rounded products, (log2 N + 2) 2^-64 of its magnitude, so
rho_j is exact to (log2 N + 2) 2^-11 < 0.007.  A column solved backward-stably with
|dA| <= C u alpha has rho_j <= C, whatever cond(A) is.  The left residual (rows of X A - I in the same
units) is not small for a solve-based inverse; it is returned to be printed, never asserted.

  Cholesky + Newton (inv_finish, :1546-1566).  These kernel matrices have a constant diagonal alpha, so
    the augmented Cholesky's |dA| <= c u alpha with the c above.  The Newton step X0 + X0 (I - A X0)
    replaces that residual by its square and by the rounding of R = I - A X0 (inv_refine_kernel<0>: the
    jitter's addition :724, a chain of k FMAs, the subtraction :782) and of X0 + X0 R (<1>: as long, one
    addition).  k = 4 ceil(N / 16) + 3 in the split-k form (N <= 1024: a quarter of the range per wave,
    :703-704, and three LDS additions, :779), k = N in the full-k form.
    C_inv = c + 2 (k + 1) + 2  ("inv-chol-splitk", "inv-chol-fullk").
  Blocked LU (bo_lu.hip) and Gauss-Jordan (gj_step_kernel, :805-864).  Partial pivoting has no a-priori
    constant without the growth factor, which is taken from the REFERENCE: growth = max |U| / max |A| of
    scipy.linalg.lu of the same f64 matrix.  The bound is C_inv growth with C_inv = 3 N + 8 ("inv-lu":
    getrf, the forward and the backward substitution, the unblocked chain lengths, which no blocking
    exceeds) and 2 N + 8 ("inv-gj": one division and one FMA per step).  The oracle, np.linalg.inv
    (getrf + getri), is held to "inv-lu".
No inverse constant may exceed 5 n_p + 64.

The tight rule, beside the hard bound on every path: the device's ratio -- err / (u S) with
S = S_chol + S_gram + S_fix for the MLL, max_j rho_j for the inverse -- must not exceed 8 R, R the
largest ratio the LAPACK oracle (oracle_np.compute_mll, np.linalg.inv) reaches over the module's cases
(mll_R, inv_R: computed on the CPU from the same reference and the same columns; 8x is DESIGN §5's rule
for a rounding term that needs naming).
"""

import numpy as np

from exact_ref import LD, LD_OK, SUBSAMPLE, U, split_ld

MP_BITS = 128
LOG_2PI = LD("1.8378770664093454835606594728112353")
TIGHT = 8.0
MAX_COLS = 48


def fit_constants(path, n, dim=0):
    """The derived constants of the module docstring: (C_chol, C_gram, C_fix) for "mll" and "oracle",
    C_inv for "inv-chol-splitk", "inv-chol-fullk", "inv-lu", "inv-gj"."""
    n_p = 32 * -(-n // 32)
    nbt = n_p // 32
    c = min(64, n_p - 32) + nbt + 38
    if path in ("mll", "oracle"):
        out = (3 * c, dim + 4, nbt + -(-n // 256) + 56) if path == "mll" else (3 * (n + 7), dim + 6, n + 16)
        assert max(out) <= 3 * n_p + 64, (path, n, out)
        return tuple(float(v) for v in out)
    if path == "inv-chol-splitk":
        assert n <= 1024
        c_inv = c + 2 * (4 * -(-n // 16) + 3 + 1) + 2
    elif path == "inv-chol-fullk":
        c_inv = c + 2 * (n + 1) + 2
    elif path == "inv-lu":
        c_inv = 3 * n + 8
    elif path == "inv-gj":
        c_inv = 2 * n + 8
    else:
        raise ValueError(path)
    assert c_inv <= 5 * n_p + 64, (path, n, c_inv)
    return float(c_inv)


# ---- the MLL

def _mll_mp(x, y_o, pm_o, ls_o, jitter, bits):
    """The reference's chain in mpmath at `bits` bits: (mll, D, Lam, w, s2) as mpf, mll None on a
    non-positive pivot."""
    import mpmath as mp
    with mp.workprec(bits):
        n = x.shape[0]
        xm = [[mp.mpf(float(v)) for v in row] for row in np.asarray(x, dtype=np.float64)]
        two_l2 = 2 * mp.mpf(float(ls_o)) ** 2
        A = [[mp.exp(-mp.fsum((p - q) ** 2 for p, q in zip(xm[i], xm[j])) / two_l2) for j in range(n)]
             for i in range(n)]
        for i in range(n):
            A[i][i] += mp.mpf(float(jitter))
        r = [mp.mpf(float(v)) - mp.mpf(float(pm_o)) for v in y_o]
        mean = mp.fsum(r) / n
        s2 = mp.fsum((v - mean) ** 2 for v in r) / n
        z = list(r)
        for j in range(n):
            if not A[j][j] > 0:
                return None, None, None, None, s2
            d = mp.sqrt(A[j][j])
            A[j][j] = d
            z[j] = z[j] / d
            for i in range(j + 1, n):
                A[i][j] = A[i][j] / d
                z[i] -= A[i][j] * z[j]
            for k in range(j + 1, n):
                for i in range(k, n):
                    A[i][k] -= A[i][j] * A[k][j]
        w = [mp.mpf(0)] * n
        for j in reversed(range(n)):
            w[j] = (z[j] - mp.fsum(A[i][j] * w[i] for i in range(j + 1, n))) / A[j][j]
        D = mp.fsum(v * v for v in z) / (s2 if s2 > 0 else 1)
        lam = 2 * mp.fsum(mp.log(A[j][j]) for j in range(n))
        return -D / 2 - lam / 2 - mp.mpf(n) / 2 * mp.log(2 * mp.pi), D, lam, w, s2


def _mll_ld(x, y_o, pm_o, ls_o, jitter):
    """The same chain in long double (a right-looking column Cholesky over the bordered matrix)."""
    n = x.shape[0]
    xl = np.asarray(x, dtype=np.float64).astype(LD)
    d = xl[:, None, :] - xl[None, :, :]
    ls = LD(float(ls_o))
    A = np.exp(-(np.einsum("ijd,ijd->ij", d, d) / (2 * ls * ls)))
    A[np.diag_indices(n)] += LD(float(jitter))
    r = np.asarray(y_o, dtype=np.float64).astype(LD) - LD(float(pm_o))
    s2 = np.mean((r - np.mean(r)) ** 2)
    z = r.copy()
    for j in range(n):
        if not A[j, j] > 0:
            return None, None, None, None, s2
        dj = np.sqrt(A[j, j])
        A[j, j] = dj
        z[j] = z[j] / dj
        if j + 1 < n:
            A[j + 1:, j] /= dj
            col = A[j + 1:, j].copy()
            z[j + 1:] -= col * z[j]
            A[j + 1:, j + 1:] -= np.outer(col, col)
    w = np.zeros(n, dtype=LD)
    for j in reversed(range(n)):
        w[j] = (z[j] - np.sum(A[j + 1:, j] * w[j + 1:])) / A[j, j]
    D = np.sum(z * z) / (s2 if s2 > 0 else LD(1))
    lam = 2 * np.sum(np.log(np.diag(A)))
    return -D / 2 - lam / 2 - LD(n) / 2 * LOG_2PI, D, lam, w, s2


def exact_mll(x, y_o, pm_o, ls_o, jitter):
    """The MLL term of one objective (module docstring) and the scales of its bound.

    Returns a dict: mll (rounded to f64; NaN on a non-positive pivot), hi, lo (the unrounded value as two
    f64), D, Lam, w, s2 (f64), S_chol, S_gram, S_fix, S (their sum: the bound at all constants 1), cond
    (of the f64 A, by eigvalsh) and n, jitter."""
    x = np.asarray(x, dtype=np.float64)
    y_o = np.asarray(y_o, dtype=np.float64)
    n = x.shape[0]
    out = dict(n=n, jitter=float(jitter))
    if LD_OK:
        mll, D, lam, w, s2 = _mll_ld(x, y_o, pm_o, ls_o, jitter)
        if mll is not None:
            out["hi"], out["lo"] = (float(v) for v in split_ld(mll))
            D, lam, s2, w = float(D), float(lam), float(s2), w.astype(np.float64)
    else:
        import mpmath as mp
        mll, D, lam, w, s2 = _mll_mp(x, y_o, pm_o, ls_o, jitter, MP_BITS)
        if mll is not None:
            with mp.workprec(MP_BITS):
                out["hi"] = float(mll)
                out["lo"] = float(mll - mp.mpf(out["hi"]))
            D, lam, s2, w = float(D), float(lam), float(s2), np.array([float(v) for v in w])
    if mll is None:
        out.update(mll=float("nan"), hi=float("nan"), lo=0.0)
        return out
    d = x[:, None, :] - x[None, :, :]
    a = np.einsum("ijd,ijd->ij", d, d) / (2.0 * float(ls_o) ** 2)
    E = np.exp(-a)
    A = E + float(jitter) * np.eye(n)
    ev = np.abs(np.linalg.eigvalsh(A))
    absinv = np.abs(np.linalg.inv(A))
    aw = np.abs(w)
    sc = s2 if s2 > 0 else 1.0
    gram = (1.0 + a) * E
    out.update(mll=out["hi"], D=D, Lam=lam, w=w, s2=s2, cond=float(ev.max() / ev.min()))
    out["S_chol"] = (1.0 + float(jitter)) * (aw.sum() ** 2 / sc + absinv.sum()) / 2.0
    out["S_gram"] = (aw @ gram @ aw / sc + float((absinv * gram).sum())) / 2.0
    out["S_fix"] = (abs(D) / 2.0 + abs(lam) / 2.0 + n / 2.0 * float(LOG_2PI) + abs(out["hi"])
                    + float(aw @ (np.abs(y_o) + abs(float(pm_o)))) / sc)
    out["S"] = out["S_chol"] + out["S_gram"] + out["S_fix"]
    return out


def mll_error(got, ref):
    """|got - the unrounded reference| in f64, through the (hi, lo) pair."""
    return float(abs((LD(float(got)) - LD(ref["hi"])) - LD(ref["lo"])))


def mll_ratio(got, ref):
    """err / (u S) at all constants 1."""
    return mll_error(got, ref) / (U * ref["S"])


def mll_tol(ref, consts):
    c_chol, c_gram, c_fix = consts
    return U * (c_chol * ref["S_chol"] + c_gram * ref["S_gram"] + c_fix * ref["S_fix"])


def check_mll(got, ref, consts, R, label=""):
    """Assert the first-order condition of the case, the hard bound and the 8 R rule on one MLL term;
    print and return its ratio."""
    assert np.isfinite(ref["mll"]), label
    assert consts[0] * U * ref["cond"] < 0.1, (label, "outside first order: a wrongly chosen case", ref["cond"])
    ratio = mll_ratio(got, ref)
    print(f"{label}: cond {ref['cond']:.1e}, err / (u S) {ratio:.3g} (8 R = {TIGHT * R:.3g}), "
          f"err / tol_hard {mll_error(got, ref) / mll_tol(ref, consts):.3g}")
    assert np.isfinite(got), (label, got)
    assert mll_error(got, ref) <= mll_tol(ref, consts), (label, "hard bound", ratio)
    assert ratio <= TIGHT * R, (label, "8 R rule", ratio, R)
    return ratio


# ---- the inverse

def sample_cols(n, seed=0):
    """At most 48 columns: the first and the last, the columns on either side of the 32-column block
    edges (all of them, or as many evenly spread edges as fit), the rest at random with a fixed seed."""
    if n <= MAX_COLS:
        return np.arange(n)
    edges = np.arange(32, n, 32)
    room = (MAX_COLS - 2) // 2
    if edges.size > room:
        edges = edges[np.unique(np.linspace(0, edges.size - 1, room).round().astype(int))]
    cols = set([0, n - 1]) | set((edges - 1).tolist()) | set(edges.tolist())
    rest = np.setdiff1d(np.arange(n), np.fromiter(cols, dtype=np.int64))
    extra = np.random.default_rng(seed).choice(rest, MAX_COLS - len(cols), replace=False)
    return np.sort(np.r_[np.fromiter(cols, dtype=np.int64), extra])


def _residual_mp(A64, X, jitter, cols, left, bits):
    import mpmath as mp
    n = A64.shape[0]
    with mp.workprec(bits):
        jit = mp.mpf(float(jitter))
        Am = [[mp.mpf(float(A64[i, k])) + (jit if i == k else 0) for k in range(n)] for i in range(n)]
        right, lft = [], []
        for j in cols:
            xj = [mp.mpf(float(v)) for v in X[:, j]]
            right.append(max(abs(mp.fsum(Am[i][k] * xj[k] for k in range(n)) - (1 if i == j else 0))
                             for i in range(n)))
            if left:
                xr = [mp.mpf(float(v)) for v in X[j, :]]
                lft.append(max(abs(mp.fsum(xr[k] * Am[k][i] for k in range(n)) - (1 if i == j else 0))
                               for i in range(n)))
        return right, lft


def exact_residual(km_o, X_o, jitter, cols, left=True, bits=None):
    """rho_j of the module docstring for the columns `cols` of X_o against K = km_o (data) + jitter I, in
    long double (mpmath at `bits` bits when given, or where long double is no wider than f64).

    Returns a dict: rho [len(cols)], left (the same ratio of row j of X A - I, or None), asym =
    max |X - X^T| / max |X|, alpha, cols."""
    K = np.asarray(km_o, dtype=np.float64)
    X = np.asarray(X_o, dtype=np.float64)
    n = K.shape[0]
    cols = np.asarray(cols)
    if not LD_OK and bits is None:
        bits, cols = MP_BITS, cols[::SUBSAMPLE]
    alpha = float(np.max(np.diag(K) + float(jitter)))
    col_1 = np.abs(X[:, cols]).sum(0)
    row_1 = np.abs(X[cols, :]).sum(1)
    if bits is not None:
        right, lft = _residual_mp(K, X, jitter, cols, left, bits)
        rho = np.array([float(v) for v in right]) / (U * alpha * col_1)
        lrat = np.array([float(v) for v in lft]) / (U * alpha * row_1) if left else None
    else:
        A = K.astype(LD)
        A[np.diag_indices(n)] += LD(float(jitter))
        At = np.ascontiguousarray(A.T) if left else None
        rho, lrat = np.empty(cols.size), (np.empty(cols.size) if left else None)
        for t, j in enumerate(cols):
            res = (A * X[:, j].astype(LD)[None, :]).sum(1)        # pairwise along the contiguous axis
            res[j] -= 1
            rho[t] = float(np.abs(res).max()) / (U * alpha * col_1[t])
            if left:
                res = (At * X[j, :].astype(LD)[None, :]).sum(1)
                res[j] -= 1
                lrat[t] = float(np.abs(res).max()) / (U * alpha * row_1[t])
    asym = float(np.abs(X - X.T).max() / np.abs(X).max())
    return dict(rho=rho, left=lrat, asym=asym, alpha=alpha, cols=cols)


def growth(km_o, jitter):
    """max |U| / max |A| of scipy.linalg.lu (getrf's partial pivoting) of the f64 K + jitter I."""
    from scipy.linalg import lu
    a = np.asarray(km_o, dtype=np.float64) + float(jitter) * np.eye(km_o.shape[0])
    return float(np.abs(lu(a, permute_l=True)[1]).max() / np.abs(a).max())


def check_inverse(res, c_inv, grow, R, label=""):
    """Assert the hard bound rho_j <= C_inv growth and the 8 R rule on exact_residual's dict; print and
    return max_j rho_j."""
    worst = float(np.max(res["rho"]))
    left = "" if res["left"] is None else f", left {float(np.max(res['left'])):.3g}"
    print(f"{label}: max rho {worst:.3g} (8 R = {TIGHT * R:.3g}, C_inv growth = {c_inv:.0f} x {grow:.3g})"
          f"{left}, asymmetry {res['asym']:.1e}")
    assert np.all(np.isfinite(res["rho"])), label
    assert worst <= c_inv * grow, (label, "hard bound", worst, c_inv, grow)
    assert worst <= TIGHT * R, (label, "8 R rule", worst, R)
    return worst


# ---- the problems that the CPU and the GPU tests share.  Every choice below is made from the inputs
# (sizes, seeds, cond of the f64 matrix on the CPU), none from a device result.

MLL_NS = (1, 2, 31, 32, 33, 64, 65, 100, 257, 513, 777)
MLL_CASES = [(n, 1e-8, "") for n in MLL_NS] + [(100, 1e-4, ""), (257, 1e-4, ""), (33, 1e-8, "std0"), (33, 1e-8, "pm")]
LAUNCH_NS = (33, 65, 100, 257, 513)
FITTED_LS = {2: 400.0, 5: 600.0}
_CACHE = {}


def _cond(x, ls, jitter, pv=1.0):
    d = x[:, None, :] - x[None, :, :]
    ev = np.abs(np.linalg.eigvalsh(pv * np.exp(-np.einsum("ijd,ijd->ij", d, d) / (2.0 * ls * ls))
                                   + jitter * np.eye(x.shape[0])))
    return float(ev.max() / ev.min())


def problem(n, dim, seed):
    """x [n, dim]: distinct points of the 1024^2 grid (dim 2) or uniform in [0, 300)^5 (dim 5, the family
    of test_gpu_fit_sweep._problem); y [n, 3]: the toy objectives plus noise; pm, pv; and the three
    length-scale classes: l1 near the point spacing with cond(E + 1e-8 I) < 1e3, 4 l1, and a fitted-like
    one."""
    rng = np.random.default_rng(seed)
    if dim == 2:
        lin = rng.choice(1024 * 1024, size=n, replace=False)
        x = np.stack([lin // 1024, lin % 1024], 1).astype(np.float64)
        extent = 1024.0
    else:
        x = rng.uniform(0, 300, size=(n, dim))
        extent = 300.0
    y = np.stack([-((x[:, o % dim] - 0.3 * extent * o) ** 2) / (extent / 6.0) + rng.normal(size=n) * 0.05
                  for o in range(3)], 1)
    pm = y.mean(0)
    pv = y.var(0) if n > 1 else np.full(3, 10.0)
    l1 = 0.8 * extent / max(1.0, n ** (1.0 / dim))
    while _cond(x, l1, 1e-8) >= 1e3:
        l1 *= 0.8
    return dict(x=x, y=y, pm=pm, pv=pv, ls=np.array([l1, 4.0 * l1, FITTED_LS[dim]]), dim=dim)


def mll_problem(key):
    """The problem of MLL_CASES' key = (n, jitter, edge): x, y, pm, pv, ls (three classes), dim, n, jitter."""
    n, jitter, edge = key
    ck = ("mll-problem",) + tuple(key)
    if ck not in _CACHE:
        p = problem(n, 5 if n in (33, 257, 777) else 2, 1000 + n)
        if edge == "std0":                     # y - pm constant (exactly: every sum below is exact), std 0
            p = dict(p, y=np.full((n, 3), 3.0), pm=np.array([1.0, 5.0, 3.0]))
        elif edge == "pm":                     # the ABI allows a prior mean that is not mean(y)
            p = dict(p, pm=p["pm"] + np.array([3.7, -11.0, 0.25]))
        _CACHE[ck] = dict(p, n=n, jitter=jitter)
    return _CACHE[ck]


def mll_case(key):
    """mll_problem(key) with its three references and the oracle's terms (oracle_np.compute_mll, one
    objective per call), computed once."""
    from oracle import oracle_np as O
    ck = ("mll",) + tuple(key)
    if ck not in _CACHE:
        p = mll_problem(key)
        n, jitter = p["n"], p["jitter"]
        refs = [exact_mll(p["x"], p["y"][:, o], p["pm"][o], p["ls"][o], jitter) for o in range(3)]
        with np.errstate(all="ignore"):
            orc = [float(O.compute_mll(p["x"], p["y"][:, o:o + 1], np.zeros((1, n, n)), p["pm"][o:o + 1],
                                       p["pv"][o:o + 1], p["ls"][o:o + 1], n, jitter=jitter)) for o in range(3)]
        _CACHE[ck] = dict(p, refs=refs, oracle=orc)
    return _CACHE[ck]


def mll_R():
    """The largest err / (u S) of oracle_np.compute_mll over MLL_CASES."""
    if "mll_R" not in _CACHE:
        _CACHE["mll_R"] = max(mll_ratio(c["oracle"][o], c["refs"][o]) for c in map(mll_case, MLL_CASES) for o in range(3))
    return _CACHE["mll_R"]


def _ls_for_cond(x, pv, jitter, target):
    """The length scale (a power of 2^(1/4) times 1) at which cond(pv E + jitter I) first reaches target."""
    ls = 1.0
    while _cond(x, ls, jitter, pv) < target and ls < 4096.0:
        ls *= 2.0 ** 0.25
    return ls


# name: (path, n, jitter, kind).  kind "chol": three objectives at l1, 4 l1 and the length scale where
# cond(K + jitter I) reaches 1e10 (an f64 Cholesky exists there with room: c u cond ~ 1e-4);
# "lu": lu_hint on every objective, 2-D grid points, l1, 4 l1 and test_gpu_lu_panels.py's fitted-regime
# l = 680 (cond > 1e16; N >= 2048: l1 and 680 only, for the reference's time); "asym": one
# non-symmetric K; "dense": one dense random matrix (a row swap at nearly every column); "fallback": no
# hint, the Cholesky is tried and fails (test_gpu_api.py's test_invert_k_lu_path_ill_conditioned: 300
# uniform points, l = 400, pv = 2e9, the fitted loop's conditioning) and the LU takes over; "gj":
# test_gpu_fit_workspace.py's Gauss-Jordan problem, one objective, well conditioned.
INV_CASES = {f"chol-n{n}": ("chol", n, 1e-6, "chol") for n in (1, 2, 33, 65, 257, 513, 1024, 1025)}
INV_CASES["chol-n257-jit1e-3"] = ("chol", 257, 1e-3, "chol")
INV_CASES.update({f"lu-n{n}": ("lu", n, 1e-6, "lu") for n in (33, 257, 512, 513, 1040, 2048)})
INV_CASES["lu-asym-n257"] = ("lu", 257, 1e-6, "asym")
INV_CASES["lu-dense-n257"] = ("lu", 257, 1e-6, "dense")
INV_CASES["lu-fallback-n300"] = ("lu", 300, 1e-6, "fallback")
INV_CASES["gj-n2049"] = ("gj", 2049, 1e-6, "gj")


def inv_path(name):
    """The constants' path of an inverse case."""
    path, n = INV_CASES[name][:2]
    return {"chol": "inv-chol-splitk" if n <= 1024 else "inv-chol-fullk", "lu": "inv-lu", "gj": "inv-gj"}[path]


def inv_km(name):
    """km [n_obj, n, n] of an inverse case: the f64 array the device is given."""
    from oracle import oracle_np as O
    ck = ("inv-km", name)
    if ck not in _CACHE:
        path, n, jitter, kind = INV_CASES[name]
        if kind == "gj":
            from test_gpu_fit_sweep import _problem
            km = _problem(n, 1, 2)[5]
        elif kind == "dense":
            km = np.random.default_rng(n).normal(size=(1, n, n))
        elif kind == "fallback":
            km = np.zeros((1, n, n))
            O.update_k(km, np.random.default_rng(4).uniform(0, 300, size=(n, 2)), 0, n, np.array([2e9]), np.array([400.0]))
        else:
            if kind == "lu" and n == 512:      # test_gpu_lu_panels.py's points
                lin = np.random.default_rng(n).choice(1024 * 1024, size=n, replace=False)
                p = dict(problem(n, 2, 2000 + n), x=np.stack([lin // 1024, lin % 1024], 1).astype(np.float64))
                while _cond(p["x"], p["ls"][0], 1e-8) >= 1e3:
                    p["ls"] = p["ls"] * np.array([0.8, 0.8, 1.0])
            else:
                p = problem(n, 5 if kind == "chol" and n in (33, 513) else 2, 2000 + n)
            ls = p["ls"].copy()
            ls[2] = 680.0 if kind == "lu" else _ls_for_cond(p["x"], p["pv"][2], jitter, 1e10)
            objs = [0, 2] if n >= 2048 else [0] if kind == "asym" else [0, 1, 2]
            km = np.zeros((len(objs), n, n))
            O.update_k(km, p["x"], 0, n, p["pv"][objs], ls[objs])
            if kind == "asym":
                km[0] *= 1.0 + 1e-3 * np.triu(np.random.default_rng(n).uniform(size=(n, n)), 1)
        _CACHE[ck] = km
    return _CACHE[ck]


def inv_case(name):
    """inv_km(name), the sampled columns, LAPACK's inverse (oracle_np.invert_k; np.linalg.inv at the other
    jitter), its residual ratios and the reference's growth factor per objective, computed once."""
    from oracle import oracle_np as O
    ck = ("inv", name)
    if ck not in _CACHE:
        path, n, jitter, kind = INV_CASES[name]
        km = inv_km(name)
        n_obj = km.shape[0]
        cols = sample_cols(n)
        inv = O.invert_k(n, km) if jitter == 1e-6 else np.stack([np.linalg.inv(k + jitter * np.eye(n)) for k in km])
        _CACHE[ck] = dict(km=km, n=n, n_obj=n_obj, jitter=jitter, cols=cols, path=path, kind=kind, oracle=inv,
                          oracle_res=[exact_residual(km[o], inv[o], jitter, cols, left=False) for o in range(n_obj)],
                          growth=[growth(km[o], jitter) for o in range(n_obj)],
                          cond=[float(np.abs(km[o] + jitter * np.eye(n)).sum(0).max() * np.abs(inv[o]).sum(0).max())
                                for o in range(n_obj)])          # the 1-norm's, from LAPACK's inverse
    return _CACHE[ck]


def inv_R():
    """The largest max_j rho_j of LAPACK's inverse over INV_CASES."""
    if "inv_R" not in _CACHE:
        _CACHE["inv_R"] = max(float(r["rho"].max()) for name in INV_CASES for r in inv_case(name)["oracle_res"])
    return _CACHE["inv_R"]

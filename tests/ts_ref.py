"""Extended-precision reference of the pathwise posterior draws (bo_sample_paths) and a rounding-error
bound for its f64 kernels.  Helper module: no tests in it (tests/test_ts_ref.py, tests/test_gpu_ts.py).

The reference.  include/bo_amd.h's definition, everything in numpy.longdouble (64-bit significand;
mpmath at 128 bits, on every SUBSAMPLE-th candidate, where the platform's long double is no wider than
f64), per objective o and draw s, with x0 = training row 0:
    w_i = Z_i / l                arg_i(c) = w_i . (c - x0) + B_i         phi_i(c) = sqrt(2 pv / D) cos(arg_i)
    g(c) = sum_i Theta_i phi_i(c)                r = y - pm - g(X) - sqrt(lam) E           v = A r
    f(c) = pm + g(c) + sum_n k(c, x_n) v_n       z(c) = (f(c) - pm) / sqrt(pv)
A = kinv is DATA (the f64 array handed to the device, as in tests/exact_ref.py), and so is v where the
caller passes one: the paths are checked with the device's OWN v (weights_out), so that the conditioning
of K enters only through tol_v and the bound on the paths holds at any cond(K).

The bound, u = 2^-53, in the form of exact_ref.py (the sums of the MAGNITUDES of the terms):
    S_g  = sum_i |Theta_i| sqrt(2 pv / D) (1 + |arg_i|)
    S_k  = sum_n (1 + a_n) k_n |v_n|,  a_n = |c - x_n|^2 / 2 l^2
    tol_f = C_f u (S_g + S_k) + 2u |f - pm|                      tol_z = tol_f / sqrt(pv) + 3u |z|
    tol_v[n] = C_v u sum_m |A_nm| (|y_m - pm| + S_g(x_m) + sqrt(lam) |E_m|)
The argument weight |arg_i| covers the cosine's argument: an absolute error u |arg_i| in the argument is
an error of that size in the cosine.

The constants are COUNTED from bayesopt_smart_amd/csrc/bo_ts.hip: the longest chain of roundings
through which one term reaches the output.
  A feature term Theta_i phi_i(c):
    the contraction: one f64 FMA per row on the matrix cores, rows in order, the D feature rows and
      then the N kernel rows in ONE accumulator (ts_paths_kernel, the two `mfma64` loops)              D + N
    the weight sqrt(2 pv / D) Theta: the quotient and the root (bo_sample_paths, `a.amp[o] =`), the
      product (ts_prep_kernel, `a.amp[o] * a.theta[...]`)                                                  3
    the cosine: cospi of the doubled argument (exact doubling, exact reduction), 2 ulp of slack           2
    the argument (|arg|-weighted): w' = (Z / l) inv_2pi (ts_prep_kernel: the quotient, the product,
      the constant's own rounding) 3, b' = B inv_2pi 1 (the constant's is counted), the centred
      coordinate c - x0 (load_centred: exact for integers) 1, one FMA per padded dimension
      (ts_paths_kernel, `tt = __builtin_fma(rp[k], c[t][k], tt)`) <= dim + 1                      dim + 6
    The FMA chain's roundings scale with its partial sums, bounded by sum_k |w_k c_k| + |B| and not by
    |arg| itself; the excess is carried by the D + N of the contraction, of which a feature term uses
    its own few.  The tests print the ratios.
  A kernel term k_n v_n (v is data):
    the contraction, as above                                                                          D + N
    K* entry by exp2_tab and lpv = log2 pv, exact_ref.py's count                                          11
    the exponent's argument (a-weighted): nl2 (bo_sample_paths, `a.nl2[o] =`) 4, the FMA sq nl2 + lpv 1,
      one difference and one FMA per dimension                                                     2 dim + 5
  C_f = N + D + 2 dim + 16, the larger of the two.  The division by sqrt(pv) (the root, the quotient) and
  the output are tol_z's 3u |z|.
  A weight v_n = sum_m A_nm r_m:
    r_m = (y - pm) - g(x_m), then the FMA with sqrt(lam) E (ts_resid_kernel) 3, sqrt(lam) itself 1        4
    g(x_m): the prior-only pass, a feature term's chain without the kernel rows: D + 3 + 2 + dim + 6
      (weighted by S_g(x_m), which is inside the sum)                                           D + dim + 11
    the mat-vec (ts_matvec_kernel): a lane's ceil(N / 64) FMAs, then the 6 additions of the xor tree
                                                                                          ceil(N / 64) + 6
  C_v = D + dim + ceil(N / 64) + 21.
Neither may exceed 2 (N + D) + 2 dim + 64; constants() asserts it.
"""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble
LD_OK = bool(np.finfo(LD).eps <= 2.0 ** -63)
SUBSAMPLE = 1 if LD_OK else 16
MP_BITS = 128


def constants(n, n_feat, dim):
    """(C_f, C_v) of the module docstring's count."""
    cf = n + n_feat + 2 * dim + 16
    cv = n_feat + dim + -(-n // 64) + 21
    cap = 2 * (n + n_feat) + 2 * dim + 64
    assert cf <= cap and cv <= cap, (cf, cv, cap)
    return float(cf), float(cv)


def rbf(a, b, pv, ls):
    d = a[:, None, :] - b[None, :, :]
    return pv * np.exp(-0.5 * np.einsum("ijk,ijk->ij", d, d) / (ls * ls))


def fitted_state(x, pv, ls, lam):
    """kinv [n_obj, N, N] = inv(K_o + lam I) in f64 and cond(K_o + lam I)."""
    n = x.shape[0]
    kinv = np.empty((len(pv), n, n))
    cond = np.empty(len(pv))
    for o in range(len(pv)):
        k = rbf(x, x, pv[o], ls[o]) + lam * np.eye(n)
        kinv[o] = np.linalg.inv(k)
        cond[o] = np.linalg.cond(k)
    return kinv, cond


def features_f64(pts, x0, z_o, b_o, pv_o, ls_o):
    """Phi [M, D] in f64: the feature map of one objective."""
    arg = (pts - x0) @ (z_o / ls_o).T + b_o
    return np.sqrt(2.0 * pv_o / z_o.shape[0]) * np.cos(arg)


def draws_f64(x, y_o, pts, pm_o, pv_o, ls_o, lam, z_o, b_o, theta_o, eps_o, kinv_o):
    """f [S, M] in f64 for one objective (theta_o [S, D], eps_o [S, N]): the definition as plain numpy,
    for statistics over thousands of draws (test_ts_ref.py pins it to the extended reference)."""
    phi_c = features_f64(pts, x[0], z_o, b_o, pv_o, ls_o)
    phi_x = features_f64(x, x[0], z_o, b_o, pv_o, ls_o)
    r = (y_o - pm_o)[None, :] - theta_o @ phi_x.T - np.sqrt(lam) * eps_o
    v = r @ kinv_o.T
    return pm_o + theta_o @ phi_c.T + v @ rbf(pts, x, pv_o, ls_o).T


def closed_form(x, y_o, pts, pm_o, pv_o, ls_o, lam, z_o, b_o, kinv_o):
    """Mean and variance of f over (Theta, E) for fixed (Z, B): pm + k kinv (y - pm) and
    |phi(c) - k(c) kinv Phi(X)|^2 + lam |k(c) kinv|^2."""
    k = rbf(pts, x, pv_o, ls_o)
    kk = k @ kinv_o
    mean = pm_o + kk @ (y_o - pm_o)
    phi_c = features_f64(pts, x[0], z_o, b_o, pv_o, ls_o)
    phi_x = features_f64(x, x[0], z_o, b_o, pv_o, ls_o)
    d = phi_c - kk @ phi_x
    return mean, np.einsum("md,md->m", d, d) + lam * np.einsum("mn,mn->m", kk, kk)


def _ld(a):
    # longdouble holds every f64 and, with a 64-bit significand, every int64 exactly
    return np.asarray(a).astype(LD)


def _prior_ld(pts, x0, z_o, b_o, pv_o, ls_o, theta_o):
    """g [M, S] (longdouble), and in f64 arg [M, D]."""
    arg = (_ld(pts) - _ld(x0)) @ (_ld(z_o) / LD(ls_o)).T + _ld(b_o)
    amp = np.sqrt(LD(2.0) * LD(pv_o) / LD(z_o.shape[0]))
    return (amp * np.cos(arg)) @ _ld(theta_o).T, arg.astype(np.float64)


def _mp_paths(x, pts, pv_o, ls_o, z_o, b_o, theta_o, v_o, exact=False):
    """f - pm [M, S] with mpmath at MP_BITS, rounded once to f64 (the fallback; pts already subsampled);
    `exact`: nested lists of mpf, unrounded."""
    import mpmath as mp
    with mp.workprec(MP_BITS):
        f = lambda a: mp.mpf(int(a)) if isinstance(a, (int, np.integer)) else mp.mpf(float(a))  # noqa: E731
        dim, nf = x.shape[1], z_o.shape[0]
        w = [[f(z_o[i, k]) / f(ls_o) for k in range(dim)] for i in range(nf)]
        amp = mp.sqrt(2 * f(pv_o) / nf)
        two_l2 = 2 * f(ls_o) ** 2
        out = [[None] * theta_o.shape[0] for _ in range(pts.shape[0])] if exact else \
            np.empty((pts.shape[0], theta_o.shape[0]))
        for m, p in enumerate(pts):
            c = [f(p[k]) - f(x[0, k]) for k in range(dim)]
            phi = [amp * mp.cos(mp.fsum(w[i][k] * c[k] for k in range(dim)) + f(b_o[i])) for i in range(nf)]
            kk = [f(pv_o) * mp.exp(-mp.fsum((f(p[k]) - f(x[n, k])) ** 2 for k in range(dim)) / two_l2)
                  for n in range(x.shape[0])]
            for s in range(theta_o.shape[0]):
                val = mp.fsum(f(theta_o[s, i]) * phi[i] for i in range(nf)) + \
                    mp.fsum(kk[n] * f(v_o[s, n]) for n in range(x.shape[0]))
                if exact:
                    out[m][s] = val
                else:
                    out[m, s] = float(val)
        return out


def weights(x, y, pm, pv, ls, lam, draws, kinv):
    """The reference's v [S, n_obj, N] (f64, rounded once from the extended value) and tol_v of the
    same shape, with kinv as data."""
    z, b, theta, eps = draws
    n, dim = x.shape
    n_s, n_obj, nf = theta.shape
    _, cv = constants(n, nf, dim)
    v = np.empty((n_s, n_obj, n))
    tol = np.empty_like(v)
    for o in range(n_obj):
        if LD_OK:
            g, arg = _prior_ld(x, x[0], z[o], b[o], pv[o], ls[o], theta[:, o])      # [N, S]
            r = (_ld(y[:, o]) - LD(pm[o]))[:, None] - g - np.sqrt(LD(lam)) * _ld(eps[:, o]).T
            v[:, o] = (_ld(kinv[o]) @ r).T.astype(np.float64)
        else:                                                    # the same chain in mpmath, rounded once
            import mpmath as mp
            arg = (x - x[0]) @ (z[o] / ls[o]).T + b[o]
            g = _mp_paths(x, x, pv[o], ls[o], z[o], b[o], theta[:, o], np.zeros((n_s, n)), exact=True)
            with mp.workprec(MP_BITS):
                for s in range(n_s):
                    r = [mp.mpf(float(y[m, o])) - mp.mpf(float(pm[o])) - g[m][s] -
                         mp.sqrt(mp.mpf(float(lam))) * mp.mpf(float(eps[s, o, m])) for m in range(n)]
                    v[s, o] = [float(mp.fsum(mp.mpf(float(kinv[o][i, m])) * r[m] for m in range(n)))
                               for i in range(n)]
        s_g = (1.0 + np.abs(arg)) @ (np.sqrt(2.0 * pv[o] / nf) * np.abs(theta[:, o])).T   # [N, S]
        mag = np.abs(y[:, o] - pm[o])[:, None] + s_g + np.sqrt(lam) * np.abs(eps[:, o]).T
        tol[:, o] = cv * U * (np.abs(kinv[o]) @ mag).T
    return v, tol


def paths(x, pts, pm, pv, ls, draws, v, full=False):
    """The reference's draws over `pts` [M, d] for the weights v [S, n_obj, N] as data.  Returns a dict
    of [S, n_obj, M] f64 arrays: z (standardised, rounded once), fc = f - pm, tol_z, tol_f -- and `sel`,
    the scored candidates' indices (every one with a wide long double, every SUBSAMPLE-th otherwise:
    the arrays then cover pts[sel]; `full`: every candidate in either case)."""
    z, b, theta, _ = draws
    n, dim = x.shape
    n_s, n_obj, nf = theta.shape
    cf, _ = constants(n, nf, dim)
    sel = np.arange(0, pts.shape[0], 1 if full else SUBSAMPLE)
    p = pts[sel]
    out = {k: np.empty((n_s, n_obj, p.shape[0])) for k in ("z", "fc", "tol_z", "tol_f")}
    for o in range(n_obj):
        d = p[:, None, :].astype(np.float64) - x[None, :, :]
        a = 0.5 * np.einsum("ijk,ijk->ij", d, d) / (ls[o] * ls[o])
        if LD_OK:
            g, arg = _prior_ld(p, x[0], z[o], b[o], pv[o], ls[o], theta[:, o])      # [M, S]
            dl = _ld(p)[:, None, :] - _ld(x)[None, :, :]
            k = LD(pv[o]) * np.exp(-np.einsum("ijk,ijk->ij", dl, dl) / (LD(2.0) * LD(ls[o]) ** 2))
            fc = g + k @ _ld(v[:, o]).T
            zz = (fc / np.sqrt(LD(pv[o]))).astype(np.float64)
            fc = fc.astype(np.float64)
        else:
            arg = (p - x[0]) @ (z[o] / ls[o]).T + b[o]
            fc = _mp_paths(x, p, pv[o], ls[o], z[o], b[o], theta[:, o], v[:, o])
            zz = fc / np.sqrt(pv[o])
        kf = pv[o] * np.exp(-a)
        s_g = (1.0 + np.abs(arg)) @ (np.sqrt(2.0 * pv[o] / nf) * np.abs(theta[:, o])).T
        s_k = ((1.0 + a) * kf) @ np.abs(v[:, o]).T
        tol_f = cf * U * (s_g + s_k) + 2 * U * np.abs(fc)
        out["fc"][:, o], out["z"][:, o], out["tol_f"][:, o] = fc.T, zz.T, tol_f.T
        out["tol_z"][:, o] = (tol_f / np.sqrt(pv[o]) + 3 * U * np.abs(zz)).T
    out["sel"] = sel
    return out


def reference(x, y, pts, pm, pv, ls, lam, draws, kinv, full=False):
    """weights() and paths() over them: the whole definition.  Adds v and tol_v to paths()'s dict."""
    v, tol_v = weights(x, y, pm, pv, ls, lam, draws, kinv)
    out = paths(x, pts, pm, pv, ls, draws, v, full)
    out["v"], out["tol_v"] = v, tol_v
    return out


# ---------------------------------------------------------------------------------- selection
def hvi_exact(p, front, ref_point):
    """HV(front u {p}) - HV(front) for every row of p [M, n_obj] (maximisation), by inclusion-exclusion
    over the front (small fronts only)."""
    from itertools import combinations
    front = np.asarray(front, dtype=np.float64).reshape(-1, len(ref_point))
    r = np.asarray(ref_point, dtype=np.float64)
    vol = np.prod(np.maximum(p - r, 0.0), axis=1)
    # volume of box(p) minus the union of the boxes box(p) n box(f): inclusion-exclusion
    for size in range(1, front.shape[0] + 1):
        for sub in combinations(range(front.shape[0]), size):
            corner = np.minimum(p, front[list(sub)].min(axis=0))
            vol = vol + (-1.0) ** size * np.prod(np.maximum(corner - r, 0.0), axis=1)
    return vol


def acquisition(z, pm, pv, kind, front=None, ref_point=None):
    """acq [S, M] of the standardised draws z [S, n_obj, M]."""
    if kind == "sum_ucb":
        return z.sum(axis=1)
    p = np.asarray(pm)[None, :, None] + np.sqrt(np.asarray(pv))[None, :, None] * z
    return np.stack([hvi_exact(p[s].T, front, ref_point) for s in range(z.shape[0])])


def best(acq, avail):
    """Index of the best available candidate in select_next_batch's order (NaN first, descending value,
    ascending index), -1 when none is left; and the gap to the next one."""
    idx = np.flatnonzero(avail)
    if idx.size == 0:
        return -1, np.inf
    a = acq[idx]
    key = np.where(np.isnan(a), np.inf, a)
    order = np.argsort(-key, kind="stable")
    gap = key[order[0]] - key[order[1]] if idx.size > 1 else np.inf
    return int(idx[order[0]]), float(gap)


def select(acq, excluded):
    """Picks [S] (local indices, -1 = none left), their values and the gaps to the next unpicked."""
    avail = ~np.asarray(excluded, dtype=bool)
    picks, vals, gaps = [], [], []
    for s in range(acq.shape[0]):
        p, g = best(acq[s], avail)
        picks.append(p)
        vals.append(acq[s, p] if p >= 0 else -np.inf)
        gaps.append(g)
        if p >= 0:
            avail[p] = False
    return np.array(picks), np.array(vals), np.array(gaps)

"""Extended-precision reference of the fused predict, and a rounding-error bound for the f64 kernels
that holds at any cond(K).  Helper module: no tests in it (tests/test_exact_ref.py, tests/test_gpu_exact.py).

The reference.  K^-1 is DATA here: the f64 array A handed to the device, used as it is (not
symmetrised, not recomputed), so that mean and quadratic form have an exact value whatever cond(K) is.
Per objective o and candidate p, everything in numpy.longdouble (64-bit significand; mpmath at 128 bits
where the platform's long double is no wider than f64):
    a_n = |p - x_n|^2 / (2 l_o^2)      k_n = pv_o exp(-a_n)       r = y_o - pm_o     alpha = A r
    mu = pm_o + k . alpha              q = k^T A k                var = max(pv_o - q, min_var)
    std_mu = (mu - pm) / sqrt(pv)      std_var = var / pv         ucb = std_mu + beta sqrt|std_var|
    acq = sum_o ucb_o                                           (oracle/oracle_np.py:150-174)

The bound.  A backward-stable evaluation of q errs by a multiple of u S_q, u = 2^-53, with
    S_q  = sum_nm (1 + a_n + a_m) k_n |A_nm| k_m          S_mu = sum_n (1 + a_n) k_n (|A| |r|)_n
-- the sums of the MAGNITUDES of the terms, which grow with the cancellation the inputs force, so the
tolerance follows the conditioning by itself.  The a weights cover the exponent's argument: a relative
error d in a_n is a relative error a_n d in k_n, the same d for every n (it does not average out).
    tol_var     = Cq  u S_q  + 2u pv          (the subtraction pv - q and the output's rounding)
    tol_mu      = Cmu u S_mu + 2u |mu|        (the addition pm + . and the output's rounding)
    tol_std_mu  = tol_mu / sqrt(pv) + 3u |std_mu|     (mu - pm, 1 / sqrt(pv), the product)
    tol_std_var = tol_var / pv + 2u                   (1 / pv, the product; std_var <= 1)
    tol_ucb_o   = acq_bound of tests/test_gpu_fp32.py with eps_mu = tol_std_mu, eps_var = tol_std_var
                  (|d sqrt v| <= min(sqrt eps, eps / sqrt v_ref); the 2u of tol_std_var carries the
                  square root's and the beta product's own rounding, 2u sqrt(v) <= 2u / sqrt(v))
                  + u |ucb_o|                         (the addition std_mu + beta sqrt)
    tol_acq     = sum_o tol_ucb_o + (n_obj - 1) u sum_o |ucb_o|      (the sum over the objectives)

What the bound leaves out.  The grid-convolution path drops a pair when |w_nm| < 2^-100 pv (kPairDrop,
bo_gridconv.hip:54): at most N (N + 1) / 2 pairs, each worth at most 2^-100 pv of q (the E factors are
<= 1), so below 2^23 2^-100 pv = 2^-77 pv at N = 4096 -- DESIGN §9.2's "q / pv below 1e-24" -- against
the 2u pv = 2^-52 pv that tol_var always holds.  The contraction's tables store entries below 2^-128
(kTabFlush, :57) as +0.0: a flushed E entry takes |T| 2^-128 <= S_q 2^-128 from q, a flushed H entry
|Tm| 2^-128 from mu, over at most 2C - 1 (N) terms: 2^-128 2^13 against u = 2^-53.  Neither needs a
term.  A change of either threshold has to redo this arithmetic: 2^-30 or 2^-40 would not pass it.

The constants Cq and Cmu are DERIVED: the longest chain of roundings through which one product reaches
the output, plus the roundings of the exponent's argument (weighted by a, hence inside S).  Counted
from the code (bayesopt_smart_amd/csrc):

"chunk-major" -- cm_predict_kernel (bo_predict_impl.h), every instantiation (small, SEP, UPPER, dense,
direct, GROWS: they differ in where rows live and how K* is generated, not in the chain), and the
unfused bo_update_k_star -> bo_update_mean_variance (bo_select.hip kstar_kernel, bo_predict.hip:19-27:
the dense chain on a materialised K*), and the two CPU oracles (one DGEMM / dot chain each):
    t = A k              N FMAs on the matrix cores (a true f64 FMA chain)            N
    k . t                N FMAs                                                                  N
    the UPPER form's entry (K^-1 + K^-T) / 2, diagonal halved (predict.py:182-184)               1
    K* entry, twice (k_n and k_m).  SEP: pv exp(sqs nhl) (bo_predict_impl.h:731: product, exp,
      product), the last-axis table exp(nhl m m) (:1183) and rv T (:528): 5 + 1 ulp of exp slack;
      direct: exp2_tab (:476-487: table entry, 4 Horner FMAs of which the last two count, the
      product) and the rounding of lpv = log2 pv (:778), |log2 pv| u ln 2 <= 8u for pv < 2^11:
      11 at most                                                                               2 x 11
    exponent's argument (a-weighted): nhl = -0.5 / (ls ls) (bo_predict.hip:811) 2, nl2 = nhl log2 e
      (:777) 2, the FMA sq nl2 + lpv (:529) 1, sqdist (:407-418) one difference and one FMA per
      dimension, 2 dim                                                                      2 dim + 5
  Cq = 2N + 2 dim + 28.      Mean: r = y - pm 1, alpha = A r N, k . alpha N, K* once 11, the argument
  as above:  Cmu = 2N + 2 dim + 17.
  One rounding is NOT of this form: the direct path centres the coordinates on training row 0 (:512-516,
  :760), so a difference carries u (|x_n - z| + |p - z|) instead of u |x_n - p|: a relative error
  (L / l) (|x_n - p| / l) u in k_n for a set of extent L.  It is exact for integer coordinates (every
  grid, every i64 set) and for dyadic ones; for f64 and Sobol sets it is bounded by the chain's slack
  while L / l < N.  The tests print the ratios; DESIGN §5 names the term.

"gridconv" -- bo_gridconv.hip, DESIGN §9.  dim = 2, integer differences (exact), cols = C:
    w_nm = sym (pv pv) exp(.) (:241-245): the sum A_nm + A_mn, pv pv, two products, exp            5
    E table entry (:369) exp, 1; the compensated T entry (two-sum and the product's FMA residual,
      DESIGN §9.2: first order in u only through the final hi + low)                           1 + 2
    the contraction's E table entry (:562)                                                         1
    the contraction over the k-blocks of tau, LT <= 2C + 14 FMAs                              2C + 14
    argument (a-weighted; the three exponents add up to a_n + a_m exactly): nhl 2, the product
      0.5 nhl (m m) 1, for each of the three factors at its own share of a_n + a_m                 3
  Cq = 2C + 2 dim + 26 (2 dim: slack kept for symmetry with the other path; no rounding stands
  behind it).      Mean: r 1, alpha = A r N (predict_prep_kernel), Tm = pv alpha exp(.) (:141) 4, the H
  table entry (:570) 1, the contraction over NP <= N + 15 FMAs, argument 3:
  Cmu = 2N + 2 dim + 24.

No constant may exceed 2 max(N, C) + 2 dim + 64 (the textbook bound of these chain lengths with slack
for the fixed terms); path_constants asserts it.
"""

import numpy as np

U = 2.0 ** -53
LD = np.longdouble
LD_OK = bool(np.finfo(LD).eps <= 2.0 ** -63)
# where long double is no wider than f64 the reference is mpmath at 128 bits, and the GPU tests score
# every SUBSAMPLE-th candidate of their samples
SUBSAMPLE = 1 if LD_OK else 16
MP_BITS = 128
OUTPUTS = ("mu", "var", "std_mu", "std_var", "ucb", "acq")


def path_constants(path, n, cols, dim):
    """(Cq, Cmu) of the module docstring's derivation.  path: "chunk-major" (every chunk-major
    instantiation, the unfused ABI, the CPU oracles) or "gridconv"; cols: the grid's last axis (C)."""
    if path == "chunk-major":
        cq, cmu = 2 * n + 2 * dim + 28, 2 * n + 2 * dim + 17
    elif path == "gridconv":
        cq, cmu = 2 * cols + 2 * dim + 26, 2 * n + 2 * dim + 24
    else:
        raise ValueError(path)
    cap = 2 * max(n, cols) + 2 * dim + 64
    assert cq <= cap and cmu <= cap, (path, cq, cmu, cap)
    return float(cq), float(cmu)


def _scales(a, k, absA, absAr):
    """S_q, S_mu [M] in f64 from a, k [M, N]."""
    ak = a * k
    t = k @ absA
    s_q = np.einsum("mn,mn->m", t, k) + np.einsum("mn,mn->m", ak @ absA, k) + np.einsum("mn,mn->m", t, ak)
    s_mu = (k + ak) @ absAr
    return s_q, s_mu


def _mp_rows(x, y_o, A, pm_o, pv_o, ls_o, pts, bits):
    """mu - pm and q per candidate with mpmath at `bits` bits: lists of mpf."""
    import mpmath as mp
    with mp.workprec(bits):
        n, dim = x.shape
        xm = [[mp.mpf(float(v)) if not isinstance(v, (int, np.integer)) else mp.mpf(int(v)) for v in row]
              for row in x]
        Am = [[mp.mpf(float(A[i, j])) for j in range(n)] for i in range(n)]
        r = [mp.mpf(float(y_o[i])) - mp.mpf(float(pm_o)) for i in range(n)]
        alpha = [mp.fsum(Am[i][j] * r[j] for j in range(n)) for i in range(n)]
        two_l2 = 2 * mp.mpf(float(ls_o)) ** 2
        pv = mp.mpf(float(pv_o))
        m_out, q_out = [], []
        for p in pts:
            pm_ = [mp.mpf(int(v)) if isinstance(v, (int, np.integer)) else mp.mpf(float(v)) for v in p]
            k = [pv * mp.exp(-mp.fsum((pm_[t] - xm[i][t]) ** 2 for t in range(dim)) / two_l2) for i in range(n)]
            m_out.append(mp.fsum(k[i] * alpha[i] for i in range(n)))
            z = [mp.fsum(Am[i][j] * k[j] for j in range(n)) for i in range(n)]
            q_out.append(mp.fsum(k[i] * z[i] for i in range(n)))
        return m_out, q_out


def exact_predict(x, y, kinv, pm, pv, ls, betas, pts, min_var=1e-10):
    """The reference of the module docstring over the candidates pts [M, d] (exactly the f64, or
    integer, values the device sees; CandidateSet.points(idx) for the device kinds).

    Returns mu, var, std_mu, std_var, ucb [n_obj, M] and acq [M] rounded to f64; S_q, S_mu [n_obj, M]
    (f64); and m_ext = mu - pm, q_ext [n_obj, M] unrounded (longdouble; with the mpmath fallback a
    pair of f64 arrays (hi, lo)) for the reference's own pinning."""
    x = np.asarray(x)
    pts = np.asarray(pts)
    y = np.asarray(y, dtype=np.float64)
    kinv = np.asarray(kinv, dtype=np.float64)
    n, n_obj, m = x.shape[0], len(pm), pts.shape[0]
    out = {k: np.empty((n_obj, m)) for k in ("mu", "var", "std_mu", "std_var", "ucb", "S_q", "S_mu")}
    out["m_ext"] = np.empty((n_obj, m), dtype=LD)
    out["q_ext"] = np.empty((n_obj, m), dtype=LD)
    # longdouble holds every f64 and, with a 64-bit significand, every int64 exactly
    d = pts.astype(LD)[:, None, :] - x.astype(LD)[None, :, :]
    sq = np.einsum("mnd,mnd->mn", d, d)
    sq64 = sq.astype(np.float64)
    acq = np.zeros(m, dtype=LD) if LD_OK else [0] * m
    for o in range(n_obj):
        A = kinv[o, :n, :n]
        r64 = (y[:n, o].astype(LD) - LD(pm[o])).astype(np.float64)
        a64 = sq64 / (2.0 * float(ls[o]) ** 2)
        absA = np.abs(A)
        out["S_q"][o], out["S_mu"][o] = _scales(a64, float(pv[o]) * np.exp(-a64), absA, absA @ np.abs(r64))
        if LD_OK:
            pm_o, pv_o, ls_o = LD(pm[o]), LD(pv[o]), LD(ls[o])
            Al = A.astype(LD)
            k = pv_o * np.exp(-(sq / (2 * ls_o * ls_o)))
            m_ext = k @ (Al @ (y[:n, o].astype(LD) - pm_o))
            q_ext = np.einsum("mn,mn->m", k @ Al.T, k)          # sum_nm k_n A_nm k_m
            mu = pm_o + m_ext
            var = np.maximum(pv_o - q_ext, LD(min_var))
            smu = (mu - pm_o) / np.sqrt(pv_o)
            svar = var / pv_o
            ucb = smu + LD(betas[o]) * np.sqrt(np.abs(svar))
            acq = acq + ucb
            for name, v in (("mu", mu), ("var", var), ("std_mu", smu), ("std_var", svar), ("ucb", ucb)):
                out[name][o] = v.astype(np.float64)
            out["m_ext"][o], out["q_ext"][o] = m_ext, q_ext
        else:                                                    # the same chain in mpmath, rounded once
            import mpmath as mp
            mm, qq = _mp_rows(x, y[:n, o], A, pm[o], pv[o], ls[o], pts, MP_BITS)
            with mp.workprec(MP_BITS):
                pm_o, pv_o, b_o = mp.mpf(float(pm[o])), mp.mpf(float(pv[o])), mp.mpf(float(betas[o]))
                for i in range(m):
                    mu = pm_o + mm[i]
                    var = max(pv_o - qq[i], mp.mpf(float(min_var)))
                    smu, svar = (mu - pm_o) / mp.sqrt(pv_o), var / pv_o
                    ucb = smu + b_o * mp.sqrt(abs(svar))
                    acq[i] = acq[i] + ucb
                    for name, v in (("mu", mu), ("var", var), ("std_mu", smu), ("std_var", svar), ("ucb", ucb)):
                        out[name][o, i] = float(v)
                    for name, v in (("m_ext", mm[i]), ("q_ext", qq[i])):
                        out[name][o, i] = LD(float(v)) + LD(float(v - mp.mpf(float(v))))
    out["acq"] = acq.astype(np.float64) if LD_OK else np.array([float(v) for v in acq])
    return out


def tolerances(ref, pv, betas, cq, cmu):
    """Per-candidate tolerances of the module docstring for every output, from exact_predict's dict."""
    from test_gpu_fp32 import acq_bound
    pv = np.asarray(pv, dtype=np.float64)
    betas = np.asarray(betas, dtype=np.float64)
    pvc = pv[:, None]
    tol = {"var": cq * U * ref["S_q"] + 2 * U * pvc,
           "mu": cmu * U * ref["S_mu"] + 2 * U * np.abs(ref["mu"])}
    tol["std_mu"] = tol["mu"] / np.sqrt(pvc) + 3 * U * np.abs(ref["std_mu"])
    tol["std_var"] = tol["var"] / pvc + 2 * U
    n_obj = pv.shape[0]
    tol["ucb"] = np.stack([acq_bound(ref["var"][o:o + 1], pv[o:o + 1], betas[o:o + 1],
                                     tol["std_mu"][o:o + 1], tol["std_var"][o:o + 1])
                           for o in range(n_obj)]) + U * np.abs(ref["ucb"])
    tol["acq"] = tol["ucb"].sum(0) + (n_obj - 1) * U * np.abs(ref["ucb"]).sum(0)
    return tol


def ratios(got, ref, tol_unit):
    """Worst err / (u scale) per output in `got`, with the scales tol_unit = tolerances(.., 1, 1):
    for var and mu that is the error in units of u S + 2u pv (u S + 2u |mu|), the figure to set
    against the constants."""
    return {k: float(np.max(np.abs(np.asarray(got[k], dtype=np.float64) - ref[k]) / tol_unit[k]))
            for k in OUTPUTS if k in got}


def check_exact(got, ref, pv, betas, cq, cmu, label=""):
    """Assert every output in `got` within its tolerance; print and return the worst ratios
    err / tolerance-at-C=1."""
    tol = tolerances(ref, pv, betas, cq, cmu)
    rat = ratios(got, ref, tolerances(ref, pv, betas, 1.0, 1.0))
    print(f"{label}: Cq {cq:.0f} Cmu {cmu:.0f}; worst err / (u scale): "
          + ", ".join(f"{k} {v:.3g}" for k, v in rat.items()))
    for name in OUTPUTS:
        if name not in got:
            continue
        g = np.asarray(got[name], dtype=np.float64)
        assert g.shape == ref[name].shape, (name, g.shape, ref[name].shape)
        err = np.abs(g - ref[name])
        bad = ~(err <= tol[name])
        assert not bad.any(), (f"{label} {name}: {int(bad.sum())} / {bad.size} beyond the bound; worst "
                               f"err / tol {float(np.nanmax(err / tol[name])):.3g} at "
                               f"{np.unravel_index(np.nanargmax(err / tol[name]), err.shape)}")
    return rat, tol


def split_ld(v):
    """A longdouble as two f64 (hi + lo exactly, for a 64-bit significand)."""
    hi = np.asarray(v, dtype=LD).astype(np.float64)
    lo = (np.asarray(v, dtype=LD) - hi.astype(LD)).astype(np.float64)
    return hi, lo


# ---- the problems that the CPU and the GPU tests share

def relength(d, ls):
    """The problem d with other length scales and K^-1 = inv(K + 1e-6 I) rebuilt (LAPACK, as the loop's
    invert_k); the worst cond(K + 1e-6 I) as d["cond"]."""
    from oracle import oracle_np as O
    x, pv = d["x"], d["pv"]
    n, n_obj = x.shape[0], len(pv)
    ls = np.broadcast_to(np.asarray(ls, dtype=np.float64), (n_obj,)).copy()
    km = np.zeros((n_obj, n, n))
    O.update_k(km, x, 0, n, pv, ls)
    out = dict(d, ls=ls, Kinv=O.invert_k(n, km))
    out["cond"] = max(float(np.linalg.cond(km[o] + 1e-6 * np.eye(n))) for o in range(n_obj))
    return out


LATTICE_A = ((37, 50), (10 ** 6, -7), 40, 2, 5)        # tests/test_gpu_gridconv.py: LATTICE
LATTICE_C = ((40, 64), (-3, 5), 130, 2, 7)
_CASES = {}


def lattice_case(name):
    """(problem, shape, lo) of the lattice cases: "a" 37 x 50, N = 40 at lattice_problem's own length
    scales (cond ~ 12); "b" the same points at ls = (7, 9) (cond 6e6 / 1.4e8); "c" 40 x 64, N = 130,
    ls = 14 (cond 3e10)."""
    import gridconv_model as G
    if name not in _CASES:
        key = LATTICE_C if name == "c" else LATTICE_A
        d = G.lattice_problem(*key)
        if name == "a":
            d = dict(d, cond=relength(d, d["ls"])["cond"])
        else:
            d = relength(d, (14.0, 14.0) if name == "c" else (7.0, 9.0))
        _CASES[name] = (d, key[0], key[1])
    return _CASES[name]

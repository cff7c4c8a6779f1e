"""Independent statement of the log-space EHVI (acquisition "logehvi"; include/bo_amd.h, bo_log_ehvi,
states the quantity), in mpmath, with the f64 restatement of the device's arithmetic, the rounding
rule's bound K and the mirror of the table form's admission rule.  numpy + scipy + mpmath only: no
device, no library.

    psi_k(a) = sigma_k h(z),  z = (mu_k - a) / sigma_k,  h(z) = phi(z) + z Phi(z),  psi_k(+inf) = 0
    F_bk     = psi_k(l_bk) - psi_k(u_bk)
    T_b      = sum_k ln F_bk
    L        = ln sum_b exp(T_b)  [ + sum_j ln P_j ,  P_j = Phi(zb_j) - Phi(za_j) ]

    rule:  |L - L_ref| <= u [C K + n_boxes + 2],  u = 2^-53,
           c(z)     = 1 + min(z, 0)^2                        (1 + z^2 for the tails of P_j)
           kappa_bk = [psi(l) c(z_l) + psi(u) c(z_u)] / F_bk
           w_b      = exp(T_b - ln sum_b exp T_b)
           K        = sum_b w_b sum_k (kappa_bk + |ln F_bk|) + sum_j (kappa_j + |ln P_j|)
    and for logpof_out alone:  |lp - lp_ref| <= u [C sum_j (kappa_j + |ln P_j|) + 2].

C = 8 (C_RULE).  MEASURED on the CPU (tests/test_logehvi_ref.py, the sweep there; scipy's erfc / erfcx):
the worst (|L - L_ref| / u - n_boxes - 2)+ / K of logehvi_f64 is 2.81 (the 4-objective case; 2.67 with one
objective at sigma = 1, z = -32.1, the first point of the series branch), of its logpof alone 1.04;
C_MEASURED records it and C_RULE is the smallest power of two that is at least twice it.
"""
import numpy as np
import mpmath as mp
from scipy import special

U = 2.0 ** -53
DPS = 60
C_MEASURED = 2.82         # worst (|L - L_ref| - u (n_boxes + 2))+ / (u K) of logehvi_f64 over the sweep
C_RULE = 8.0              # the smallest power of two >= 2 C_MEASURED; the device is held to it
T_SERIES = 32.0           # |z| at and above which B comes from the series in 1 / z^2
T_TAIL = 6.0              # the nearer tail argument at and above which ln P is assembled from ln Q
LDS_BYTES = 160 * 1024    # bo_ehvi_impl.h: kEhviLdsBytes
TABLE_THREADS = (256, 128, 64)
EDGE_BYTES = 16           # one extended-range psi per edge and thread: an f64 mantissa, an f64 exponent
SERIES = (1.0, -3.0, 15.0, -105.0, 945.0, -10395.0, 135135.0, -2027025.0, 34459425.0)
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
RSQRT2PI = 0.3989422804014327
RSQRT2 = 0.7071067811865476


def table_threads(sum_edges):
    """Mirror of bo_logehvi_table_threads: the table holds 16 sum_edges bytes per thread; the workgroup
    is the largest T of TABLE_THREADS whose table fits the LDS of a CU; 0 when none does."""
    if sum_edges < 0:
        return 0
    for t in TABLE_THREADS:
        if EDGE_BYTES * sum_edges * t <= LDS_BYTES:
            return t
    return 0


# ------------------------------------------------------------------------------- mpmath
def _dps_for(z):
    """phi + z Phi cancels to 1 / z^2 of its terms for z < 0: digits on top of DPS so that DPS remain."""
    az = abs(float(z)) if mp.isfinite(z) else 1.0
    return DPS + 8 + 2 * int(np.ceil(np.log10(max(az, 1.0))))


def psi_mp(mu, var, a):
    """(psi, c): psi = E[(Y - a)+] as an mpf from f64 mu, var, a, and c = 1 + min(z, 0)^2 (1 where psi
    is a limit).  sigma = sqrt(|var|) unrounded."""
    if a == np.inf:
        return mp.mpf(0), mp.mpf(1)
    mu, var, a = mp.mpf(float(mu)), mp.mpf(float(var)), mp.mpf(float(a))
    d = mu - a
    if var == 0 or not mp.isfinite(d):
        return (d if d > 0 else mp.mpf(0)), mp.mpf(1)
    sigma = mp.sqrt(abs(var))
    z = d / sigma
    with mp.workdps(_dps_for(z)):
        if z >= 0:
            h = mp.npdf(z) + z * (1 - mp.erfc(z / mp.sqrt(2)) / 2)
            c = mp.mpf(1)
        else:
            h = mp.npdf(z) + z * mp.erfc(-z / mp.sqrt(2)) / 2
            c = 1 + z * z
        psi = sigma * h
    return +psi, +c


def ln_pof_mp(mu, var, lo, hi):
    """(ln P, kappa) of one constraint: P = Phi(zb) - Phi(za) as a difference of tail terms, kappa = [Q1 (1 +
    z1^2) + Q2 (1 + z2^2)] / P over the two tail terms.  P = 0 gives (-inf, 0)."""
    mu, var = mp.mpf(float(mu)), mp.mpf(float(var))
    if var == 0:
        return (mp.mpf(0) if lo <= mu <= hi else -mp.inf), mp.mpf(0)
    sigma = mp.sqrt(abs(var))

    def zq(bound, sign):            # the tail term Q(sign (bound - mu) / sigma) and its c
        if np.isinf(bound):
            z = mp.inf if sign * bound > 0 else -mp.inf
            return z, (mp.mpf(0) if z > 0 else mp.mpf(1))
        z = sign * (mp.mpf(float(bound)) - mu) / sigma
        return z, mp.erfc(z / mp.sqrt(2)) / 2

    za, _ = zq(lo, 1)
    zb, _ = zq(hi, 1)
    with mp.workdps(DPS + 10):
        if za > 0:
            (z1, q1), (z2, q2) = zq(lo, 1), zq(hi, 1)
            p = q1 - q2
        elif zb < 0:
            (z1, q1), (z2, q2) = zq(hi, -1), zq(lo, -1)
            p = q1 - q2
        else:
            (z1, q1), (z2, q2) = zq(hi, 1), zq(lo, -1)
            p = 1 - q1 - q2
        if p <= 0:
            return -mp.inf, mp.mpf(0)
        kap = mp.mpf(0)
        for z, q in ((z1, q1), (z2, q2)):
            if q != 0:
                kap += q * (1 + z * z)
        return mp.log(p), kap / p


def box_part(mu, var, boxes):
    """Per candidate, from the objective rows alone: None where a row holds NaN, else (lse, kbox) with lse =
    ln sum_b exp T_b (None when no box has all factors positive) and kbox = sum_b w_b sum_k (kappa_bk + |ln F_bk|)."""
    mu = np.asarray(mu, dtype=np.float64)
    var = np.asarray(var, dtype=np.float64)
    m, n = mu.shape
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 2 * m)
    out = []
    with mp.workdps(DPS):
        for i in range(n):
            if np.isnan(mu[:, i]).any() or np.isnan(var[:, i]).any():
                out.append(None)
                continue
            cache = {}

            def p(k, a):
                if (k, a) not in cache:
                    cache[(k, a)] = psi_mp(mu[k, i], var[k, i], a)
                return cache[(k, a)]

            terms = []                                   # (T_b, sum_k kappa + |ln F|)
            for b in boxes:
                t, kb = mp.mpf(0), mp.mpf(0)
                for k in range(m):
                    (pl, cl), (pu, cu) = p(k, b[k]), p(k, b[m + k])
                    f = pl - pu
                    if f <= 0:
                        t = None
                        break
                    lf = mp.log(f)
                    t += lf
                    kb += (pl * cl + pu * cu) / f + abs(lf)
                if t is not None:
                    terms.append((t, kb))
            if not terms:
                out.append((None, None))
                continue
            tmax = max(t for t, _ in terms)
            lse = tmax + mp.log(mp.fsum(mp.exp(t - tmax) for t, _ in terms))
            out.append((lse, mp.fsum(mp.exp(t - lse) * kb for t, kb in terms)))
    return out


def con_part(mu, var, bounds):
    """Per constraint row j and candidate i: None where the row holds NaN there, else ln_pof_mp's (ln P, kappa)."""
    mu = np.asarray(mu, dtype=np.float64)
    var = np.asarray(var, dtype=np.float64)
    with mp.workdps(DPS):
        return [[None if np.isnan(mu[j, i]) or np.isnan(var[j, i]) else ln_pof_mp(mu[j, i], var[j, i], lo, hi)
                 for i in range(mu.shape[1])] for j, (lo, hi) in enumerate(bounds)]


def combine(box, con, n_boxes, c=C_RULE):
    """(L_ref, bound, lp_ref, lp_bound) of the rule from box_part's and (a prefix of) con_part's output."""
    n = len(box)
    L, bnd, lp, lpb = np.empty(n), np.empty(n), np.empty(n), np.empty(n)
    with mp.workdps(DPS):
        for i in range(n):
            if any(row[i] is None for row in con):       # NaN in a constraint row: both are NaN
                L[i] = lp[i] = np.nan
                bnd[i] = lpb[i] = 0.0
                continue
            lpi, kc = mp.mpf(0), mp.mpf(0)
            for row in con:
                l, kap = row[i]
                lpi += l
                if l != -mp.inf:
                    kc += kap + abs(l)
            lp[i] = float(lpi)
            lpb[i] = float(U * (c * kc + 2)) if lpi != -mp.inf else 0.0
            if box[i] is None:                           # NaN in an objective row: L is NaN, logpof is not
                L[i], bnd[i] = np.nan, 0.0
            elif box[i][0] is None or lpi == -mp.inf:
                L[i], bnd[i] = -np.inf, 0.0
            else:
                L[i] = float(box[i][0] + lpi)
                bnd[i] = float(U * (c * (box[i][1] + kc) + n_boxes + 2))
    return L, bnd, lp, lpb


def reference(mu, var, boxes, bounds=None, c=C_RULE):
    """(L_ref [n], bound [n], lp_ref [n], lp_bound [n]) of the rule from f64 mu / var [n_obj + n_con, n] (the
    objective rows first), boxes [n_boxes, 2 n_obj] (hypervolume_boxes' layout) and bounds [n_con, 2].
    Where a reference value is not finite (NaN, -inf: the limits) its bound is 0: the device must give
    that value."""
    mu = np.asarray(mu, dtype=np.float64)
    var = np.asarray(var, dtype=np.float64)
    bounds = np.zeros((0, 2)) if bounds is None else np.asarray(bounds, dtype=np.float64).reshape(-1, 2)
    m = mu.shape[0] - bounds.shape[0]
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 2 * m)
    return combine(box_part(mu[:m], var[:m], boxes), con_part(mu[m:], var[m:], bounds), boxes.shape[0], c)


def check_rule(got, ref, bound):
    """The share of candidates that miss the rule, and the worst |error| / bound."""
    got = np.asarray(got, dtype=np.float64)
    fin = np.isfinite(ref)
    same = np.where(np.isnan(ref), np.isnan(got), got == ref)
    with np.errstate(all="ignore"):
        err = np.abs(got - ref)
        ok = np.where(fin, err <= bound, same)
        ratio = np.where(fin, err / bound, 0.0)
    return 1.0 - ok.mean(), float(ratio.max()) if ratio.size else 0.0


# ------------------------------------------------------------------------------- f64 restatement
def _frexp(v):
    m, e = np.frexp(v)
    return m, e.astype(np.float64)


def psi_ext_f64(mu, sigma, a):
    """The device's extended-range psi (m, e), psi = m 2^e, restated in f64: arrays mu, sigma; scalar a.
    Zero is (0, 0).  d >= 0: max(d, 0) + sigma h(|z|) in f64 (bo_ehvi_impl.h's psi), split by frexp.
    d < 0: B(t) = h(t) exp(t^2 / 2) from the erfcx form (t < 32) or the series in 1 / t^2, the exponent
    -t^2 / 2 log2(e) split into its integer and its fraction."""
    mu = np.asarray(mu, dtype=np.float64)
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float64), mu.shape)
    if np.isposinf(a):
        return np.zeros(mu.shape), np.zeros(mu.shape)
    with np.errstate(all="ignore"):
        d = mu - a
        rs = 1.0 / sigma
        t = np.abs(d * rs)
        # d >= 0
        hp = np.where(t < 40.0, np.exp(-0.5 * (t * t)) * (RSQRT2PI - (0.5 * t) * special.erfcx(t * RSQRT2)), 0.0)
        vp = sigma * hp + np.maximum(d, 0.0)
        mp_, ep_ = _frexp(np.where(np.isfinite(vp), vp, 0.0))
        # d < 0
        t2 = t * t
        w = 1.0 / t2
        ser = np.full(mu.shape, SERIES[-1])
        for cf in SERIES[-2::-1]:
            ser = cf + w * ser
        bb = np.where(t < T_SERIES, RSQRT2PI - (0.5 * t) * special.erfcx(t * RSQRT2), (RSQRT2PI * w) * ser)
        x = (-0.5 * t2) * LOG2E
        ei = np.rint(x)
        mb, eb = _frexp(bb * np.exp2(x - ei))
        ms, es = _frexp(sigma)
        mn, en = mb * ms, ei + (eb + es)
        dead = ~(t2 < 1e300) | ~(mn > 0.0)
        mn, en = np.where(dead, 0.0, mn), np.where(dead, 0.0, en)
        # sigma = 0
        m0, e0 = _frexp(np.maximum(np.where(np.isfinite(d), d, 0.0), 0.0))
    neg = d < 0.0
    zero = sigma == 0.0
    m = np.where(zero, m0, np.where(neg, mn, mp_))
    e = np.where(zero, e0, np.where(neg, en, ep_))
    return m, e


def _ldexp(m, de):
    return np.ldexp(m, np.clip(de, -2000.0, 2000.0).astype(np.int64))


def ln_pof_f64(mu, sigma, lo, hi):
    """ln P(lo <= Y <= hi) as the device evaluates it.  za > 0 (zb < 0 mirrored), with t1 <= t2 the two
    tails' arguments: ln(Q(t1) - Q(t2)) for t1 < 6, where Q is far from its underflow; from there on
    ln Q(t1) + ln(-expm1(ln Q(t2) - ln Q(t1))), the difference of the logarithms as ln(erfcx ratio) -
    (t2 - t1)(t2 + t1) / 2; otherwise log1p(-(Q(zb) + Q(-za)))."""
    mu = np.asarray(mu, dtype=np.float64)
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float64), mu.shape)
    with np.errstate(all="ignore"):
        za = (lo - mu) / sigma
        zb = (hi - mu) / sigma
        above = za > 0.0
        below = ~above & (zb < 0.0)
        t1 = np.where(above, za, np.where(below, -zb, zb))
        t2 = np.where(above, zb, -za)
        # the tail branches: 0 <= t1 <= t2
        l1 = np.log(0.5 * special.erfcx(t1 * RSQRT2))
        l2 = np.log(0.5 * special.erfcx(t2 * RSQRT2))
        dl = (l2 - l1) - (0.5 * (t2 - t1)) * (t2 + t1)
        dl = np.where(np.isposinf(t2), -np.inf, dl)
        far = (l1 - 0.5 * (t1 * t1)) + np.log(-np.expm1(dl))
        # the tail branches below T_TAIL, and the central branch: Q itself
        q1 = 0.5 * special.erfc(t1 * RSQRT2)
        q2 = 0.5 * special.erfc(t2 * RSQRT2)
        near = np.log(q1 - q2)
        cen = np.log1p(-(q1 + q2))
        out = np.where(above | below, np.where(t1 < T_TAIL, near, far), cen)
    out = np.where(sigma == 0.0, np.where((lo <= mu) & (mu <= hi), 0.0, -np.inf), out)
    return np.where(np.isnan(mu) | np.isnan(sigma), np.nan, out)


def logehvi_f64(mu, var, boxes, bounds=None):
    """(L [n], lp [n]): the device's arithmetic in f64 numpy (scipy's erfc / erfcx, numpy's exp, exp2, log):
    extended-range psi per bound, F = max(m_l - m_u 2^(e_u - e_l), 0) at exponent e_l, the product left to
    right over k renormalised by frexp, the running sum aligned to the running maximum exponent in box
    order, L = e ln 2 + ln m, then + lp = ((ln P_0 + ln P_1) + ...)."""
    mu = np.asarray(mu, dtype=np.float64)
    var = np.asarray(var, dtype=np.float64)
    bounds = np.zeros((0, 2)) if bounds is None else np.asarray(bounds, dtype=np.float64).reshape(-1, 2)
    n_con = bounds.shape[0]
    m = mu.shape[0] - n_con
    n = mu.shape[1]
    sigma = np.sqrt(np.abs(var))
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 2 * m)
    cache = {}

    def p(k, a):
        if (k, a) not in cache:
            cache[(k, a)] = psi_ext_f64(mu[k], sigma[k], a)
        return cache[(k, a)]

    sm, se = np.zeros(n), np.full(n, -np.inf)
    with np.errstate(all="ignore"):
        for b in boxes:
            vm, ve = np.ones(n), np.zeros(n)
            for k in range(m):
                (ml, el), (mu_, eu) = p(k, b[k]), p(k, b[m + k])
                f = np.maximum(ml - _ldexp(mu_, eu - el), 0.0)
                vm, ve = (f, el) if k == 0 else (vm * f, ve + el)
            vm, dv = _frexp(vm)
            ve = ve + dv
            on = vm > 0.0
            e = np.maximum(se, ve)
            new = _ldexp(sm, np.where(on, se - e, 0.0)) + _ldexp(vm, np.where(on, ve - e, 0.0))
            sm, se = np.where(on, new, sm), np.where(on, e, se)
        L = np.where(sm > 0.0, se * LN2 + np.log(sm), -np.inf)
        lp = np.zeros(n)
        for j in range(n_con):
            lj = ln_pof_f64(mu[m + j], sigma[m + j], bounds[j, 0], bounds[j, 1])
            lp = lj if j == 0 else lp + lj
        L = L + lp if n_con else L
    nan = np.isnan(mu).any(axis=0) | np.isnan(var).any(axis=0)
    return np.where(nan, np.nan, L), np.where(np.isnan(mu[m:]).any(axis=0) | np.isnan(var[m:]).any(axis=0), np.nan, lp)


def select_top(values, excluded, q):
    """The q best non-excluded candidates (NaN absent; descending value, ties by ascending index) and the gaps
    between consecutive values of that order (q of them: the last against the best unpicked one)."""
    v = np.where(excluded, -np.inf, np.asarray(values, dtype=np.float64))
    order = np.argsort(-v, kind="stable")
    with np.errstate(invalid="ignore"):
        gaps = v[order[:q]] - v[order[1:q + 1]]
    return order[:q], gaps, order[1:q + 1]


# ------------------------------------------------------------------------------- the motivating case
GRID_LO, GRID_SHAPE = (-5, 100), (33, 31)
MOTIVATING_SEED = 3


def grid_points():
    a = np.arange(GRID_LO[0], GRID_LO[0] + GRID_SHAPE[0], dtype=np.float64)
    b = np.arange(GRID_LO[1], GRID_LO[1] + GRID_SHAPE[1], dtype=np.float64)
    return np.stack(np.meshgrid(a, b, indexing="ij"), -1).reshape(-1, 2)


def motivating_case(seed=MOTIVATING_SEED, n_train=120, length_scale=200.0):
    """The state a fitted loop lives in: the 33 x 31 grid, two smooth objectives (negative quadratic bowls
    centred at (0.3, 0.4) and (0.7, 0.6) of the box), n_train evaluated grid points drawn with `seed`, a GP
    posterior per objective with prior mean = mean(y), prior variance = var(y), one long length scale,
    jitter 1e-6 and the variance floored at 1e-10; reference point = the per-objective minimum - 0.1.
    Returns dict(mu, var [2, 1023], front, ref_point, evaluated (bool [1023]), y)."""
    pts = grid_points()
    ab = (pts - np.array(GRID_LO, dtype=np.float64)) / (np.array(GRID_SHAPE, dtype=np.float64) - 1.0)
    f = np.stack([-(ab[:, 0] - 0.3) ** 2 - (ab[:, 1] - 0.4) ** 2, -(ab[:, 0] - 0.7) ** 2 - (ab[:, 1] - 0.6) ** 2])
    rng = np.random.default_rng(seed)
    tr = np.sort(rng.choice(pts.shape[0], n_train, replace=False))
    x, y = pts[tr], f[:, tr]
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    ds = ((pts[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    mu, var = np.empty((2, pts.shape[0])), np.empty((2, pts.shape[0]))
    for k in range(2):
        pm, pv = y[k].mean(), y[k].var()
        kk = pv * np.exp(-0.5 * d2 / length_scale ** 2) + 1e-6 * np.eye(n_train)
        ks = pv * np.exp(-0.5 * ds / length_scale ** 2)
        kinv = np.linalg.inv(kk)
        mu[k] = pm + ks @ (kinv @ (y[k] - pm))
        var[k] = np.maximum(pv - np.einsum("ij,jk,ik->i", ks, kinv, ks), 1e-10)
    yt = y.T
    dom = ((yt[None, :, :] >= yt[:, None, :]).all(-1) & (yt[None, :, :] > yt[:, None, :]).any(-1)).any(1)
    front = yt[~dom]
    evaluated = np.zeros(pts.shape[0], dtype=bool)
    evaluated[tr] = True
    return {"mu": mu, "var": var, "front": front, "ref_point": y.min(axis=1) - 0.1, "evaluated": evaluated,
            "y": yt, "points": pts}


def boxes_2d(front, ref_point):
    """The disjoint boxes of the region above ref_point that no row of front (2 objectives, mutually
    non-dominated, above ref_point) dominates, in hypervolume_boxes' layout: vertical strips by descending
    first objective.  A host-only stand-in for bo_hvi_boxes in the reference-only tests."""
    f = np.asarray(front, dtype=np.float64).reshape(-1, 2)
    f = f[np.argsort(-f[:, 0], kind="stable")]
    out, hi = [], np.inf
    lo1 = float(ref_point[1])
    for a, b in f:
        out.append([a, lo1, hi, np.inf])
        hi, lo1 = a, b
    out.append([float(ref_point[0]), lo1, hi, np.inf])
    return np.array(out, dtype=np.float64)

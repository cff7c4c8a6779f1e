"""The EHVI and the constrained EHVI (acquisition "ehvi"; bo_expected_hypervolume_improvement and
bo_constrained_ehvi of include/bo_amd.h) in mpmath at 60 digits, the rounding rule they are held to, and
the f64 restatement of the device's arithmetic (bo_ehvi_impl.h: ehvi_psi, ehvi_direct_value, ehvi_pof) that
measures the rule's constant.  numpy + scipy + mpmath only: no device, no library.  psi and P come from
tests/logehvi_ref.py (psi_mp, ln_pof_mp), which states them from the f64 inputs with their conditioning.

    psi_k(a) = E[(Y_k - a)+],  Y_k ~ N(mu_k, |var_k|),  c(z) = 1 + min(z, 0)^2,  z = (mu_k - a) / sigma_k
    F_bk     = psi_k(l_bk) - psi_k(u_bk)  (>= 0)        kappa_bk = [psi(l) c(z_l) + psi(u) c(z_u)] / F_bk
    T_b      = prod_k F_bk                              E_ref    = sum_b T_b
    Kbox     = sum_b T_b sum_k kappa_bk
    P_ref    = prod_j P_j,  P_j = P(lo_j <= Y_j <= hi_j)    Kcon = sum_j kappa_j  (ln_pof_mp's)

    the plain scan:           |E - E_ref|       <= bound_E = u [C Kbox + (n_boxes + n_obj + 1) E_ref]
    the constrained scan:     |V - E_ref P_ref| <= P_ref bound_E + E_ref P_ref u [C Kcon + n_con + 1]
    pof_out alone:            |P - P_ref|       <= P_ref u [C Kcon + n_con + 1]              u = 2^-53

Every bound is u (C k + base): Rule holds k and base per candidate, so that one sweep measures the C a
set of values needs.  Where the reference is NaN or exactly 0 the bound is 0 and the value must be met;
where it is positive but below 2^-900 (LOW) an f64 product of psi's has no relative precision left and the
value need only lie in [0, 2^-899].  A case keeps every F_bk <= 2^10 (F_MAX), so that the absolute error of
a subnormal psi carried through the product stays far under u 2^-900, and at most 5 % (LOW_SHARE) of its
candidates below LOW: Rule.qualifies.

C = 16 (C_RULE).  MEASURED on the CPU (tests/test_ehvi_exact_ref.py, the sweep there; scipy's erfc / erfcx):
the worst (|E - E_ref| / u - (n_boxes + n_obj + 1) E_ref)+ / Kbox of ehvi_f64 is 4.55 (one objective, sigma^2 =
1e-10), of pof_f64 alone 1.57, of the product 4.52; C_MEASURED records it and C_RULE is the smallest power of
two that is at least twice it.
"""
import numpy as np
import mpmath as mp
from scipy import special

from logehvi_ref import DPS, U, ln_pof_mp, psi_mp

C_MEASURED = 4.56         # worst (|err| / u - base)+ / k of ehvi_f64 / pof_f64 / cehvi_f64 over the sweep
C_RULE = 16.0             # the smallest power of two >= 2 C_MEASURED; the device is held to it
LOW = mp.ldexp(1, -900)   # below it the relative rule does not apply
LOW_CAP = 2.0 ** -899     # ... and the value lies in [0, LOW_CAP]
LOW_SHARE = 0.05
F_MAX = 2.0 ** 10
CUTOFF = 40.0             # bo_ehvi_impl.h: h(t) = 0 from t = 40 on
RSQRT2PI = 0.3989422804014327
RSQRT2 = 0.7071067811865476


class Rule:
    """One quantity's reference and bound per candidate: ref[i] an mpf, or None for NaN; bound[i] =
    u (c k[i] + base[i])."""

    def __init__(self, ref, k, base, c, fmax=0.0):
        self.ref, self.k, self.base, self.c, self.fmax = ref, k, base, c, fmax
        self.nan = np.array([r is None for r in ref], dtype=bool)
        self.zero = np.array([r is not None and r == 0 for r in ref], dtype=bool)
        self.low = np.array([r is not None and 0 < r < LOW for r in ref], dtype=bool)
        self.held = ~(self.nan | self.zero | self.low)             # where the relative rule applies
        self.val = np.array([np.nan if r is None else float(r) for r in ref], dtype=np.float64)
        with mp.workdps(DPS):
            self.bound = np.array([float(U * (c * kk + bb)) if h else 0.0 for kk, bb, h in zip(k, base, self.held)])

    def __len__(self):
        return len(self.ref)

    def head(self, n):
        return Rule(self.ref[:n], self.k[:n], self.base[:n], self.c, self.fmax)

    def qualifies(self):
        """The two conditions every case meets, on the reference alone."""
        return self.fmax <= F_MAX and self.low.mean() <= LOW_SHARE

    def _errors(self, got):
        """(exact [n] bool: the limits are met, err [n] mpf or None: |got - ref| where the rule applies)."""
        got = np.asarray(got, dtype=np.float64)
        assert got.shape == (len(self.ref),)
        with np.errstate(invalid="ignore"):
            exact = np.where(self.nan, np.isnan(got), np.where(self.zero, got == 0.0,
                             np.where(self.low, (got >= 0.0) & (got <= LOW_CAP), np.isfinite(got))))
        with mp.workdps(DPS):
            err = [abs(mp.mpf(float(g)) - r) if h and np.isfinite(g) else None for g, r, h in zip(got, self.ref, self.held)]
        return exact, err

    def check(self, got):
        """(the number of candidates that miss the rule or a limit, the worst |got - ref| / bound)."""
        exact, err = self._errors(got)
        miss, worst = int((~exact).sum()), 0.0
        with mp.workdps(DPS):
            for e, kk, bb in zip(err, self.k, self.base):
                if e is None:
                    continue
                b = U * (self.c * kk + bb)
                if e > b:
                    miss += 1
                worst = max(worst, float(e / b) if b > 0 else (0.0 if e == 0 else np.inf))
        return miss, worst

    def c_needed(self, got):
        """The smallest C with which `got` meets the rule: the worst (err / u - base)+ / k; inf where a
        limit is missed or k = 0 leaves an excess."""
        exact, err = self._errors(got)
        if not exact.all():
            return np.inf
        worst = 0.0
        with mp.workdps(DPS):
            for e, kk, bb in zip(err, self.k, self.base):
                if e is None:
                    continue
                extra = e / U - bb
                if extra > 0:
                    worst = max(worst, float(extra / kk) if kk > 0 else np.inf)
        return worst


# ------------------------------------------------------------------------------- mpmath
def box_part(mu, var, boxes):
    """Per candidate, from the objective rows alone: None where a row holds NaN, else (E_ref, Kbox); and the
    largest F_bk met."""
    mu = np.asarray(mu, dtype=np.float64)
    var = np.asarray(var, dtype=np.float64)
    m, n = mu.shape
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 2 * m)
    out, fmax = [], mp.mpf(0)
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

            e, kbox = mp.mpf(0), mp.mpf(0)
            for b in boxes:
                t, kap = mp.mpf(1), mp.mpf(0)
                for k in range(m):
                    (pl, cl), (pu, cu) = p(k, b[k]), p(k, b[m + k])
                    f = pl - pu
                    if f <= 0:                            # the exact value is >= 0: an empty or unreachable box
                        t = mp.mpf(0)
                        break
                    fmax = max(fmax, f)
                    t *= f
                    kap += (pl * cl + pu * cu) / f
                e += t
                kbox += t * kap
            out.append((e, kbox))
    return out, float(fmax)


def con_part(mu, var, bounds):
    """Per constraint row j and candidate i: None where the row holds NaN there, else (P_j, kappa_j)."""
    mu = np.asarray(mu, dtype=np.float64)
    var = np.asarray(var, dtype=np.float64)
    out = []
    with mp.workdps(DPS):
        for j, (lo, hi) in enumerate(bounds):
            row = []
            for i in range(mu.shape[1]):
                if np.isnan(mu[j, i]) or np.isnan(var[j, i]):
                    row.append(None)
                    continue
                lp, kap = ln_pof_mp(mu[j, i], var[j, i], lo, hi)
                row.append((mp.exp(lp) if lp != -mp.inf else mp.mpf(0), kap))
            out.append(row)
    return out


def combine(box, con, n_boxes, n_obj, c=C_RULE):
    """(E, P, V): the Rules of the plain scan, of pof_out and of the constrained scan's value, from
    box_part's and (a prefix of) con_part's output."""
    (box, fmax), n_con = box, len(con)
    n = len(box)
    e_ref, e_k, e_b, p_ref, p_k, p_b, v_ref, v_k, v_b = ([] for _ in range(9))
    zero = mp.mpf(0)
    with mp.workdps(DPS):
        for i in range(n):
            if box[i] is None:
                e, kbox, eb = None, zero, zero
            else:
                e, kbox = box[i]
                eb = (n_boxes + n_obj + 1) * e
            if any(row[i] is None for row in con):
                p, kcon = None, zero
            else:
                p, kcon = mp.mpf(1), zero
                for row in con:
                    p *= row[i][0]
                    kcon += row[i][1]
            e_ref.append(e), e_k.append(kbox), e_b.append(eb)
            p_ref.append(p), p_k.append(zero if p is None else p * kcon), p_b.append(zero if p is None else p * (n_con + 1))
            if e is None or p is None:
                v_ref.append(None), v_k.append(zero), v_b.append(zero)
            else:
                v_ref.append(e * p), v_k.append(p * kbox + e * p * kcon), v_b.append(p * eb + e * p * (n_con + 1))
    return Rule(e_ref, e_k, e_b, c, fmax), Rule(p_ref, p_k, p_b, c), Rule(v_ref, v_k, v_b, c, fmax)


def reference(mu, var, boxes, bounds=None, c=C_RULE):
    """(E, P, V) Rules from f64 mu / var [n_obj + n_con, n] (the objective rows first), boxes [n_boxes,
    2 n_obj] (hypervolume_boxes' layout) and bounds [n_con, 2].  Without constraints P is 1 and V is E."""
    mu = np.asarray(mu, dtype=np.float64)
    var = np.asarray(var, dtype=np.float64)
    bounds = np.zeros((0, 2)) if bounds is None else np.asarray(bounds, dtype=np.float64).reshape(-1, 2)
    m = mu.shape[0] - bounds.shape[0]
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 2 * m)
    return combine(box_part(mu[:m], var[:m], boxes), con_part(mu[m:], var[m:], bounds), boxes.shape[0], m, c)


def boxes_one_point(point, ref_point):
    """m + 1 disjoint boxes, in hypervolume_boxes' layout, of the region above ref_point that the one point
    does not dominate (m >= 2 objectives): box k holds what exceeds the point in objective k and in none
    before it, [r_j, f_j) for j < k, [f_k, inf), [r_j, inf) for j > k; the first of them is cut in two at
    the point's last coordinate along the last objective, so that every objective meets a finite upper edge
    and two boxes share one.  A host-only stand-in for bo_hvi_boxes in the reference-only tests."""
    f = np.asarray(point, dtype=np.float64).ravel()
    r = np.asarray(ref_point, dtype=np.float64).ravel()
    m = f.size
    assert m >= 2 and (f > r).all()
    out = []
    for k in range(m):
        lo = np.concatenate([r[:k], f[k:k + 1], r[k + 1:]])
        hi = np.concatenate([f[:k], np.full(m - k, np.inf)])
        out.append(np.concatenate([lo, hi]))
    first = out.pop(0)
    below, above = first.copy(), first.copy()
    below[2 * m - 1] = f[m - 1]
    above[m - 1] = f[m - 1]
    return np.array([below, above] + out, dtype=np.float64)


# ------------------------------------------------------------------------------- f64 restatement
def psi_f64(mu, sigma, a, erfcx=special.erfcx, cutoff=CUTOFF):
    """ehvi_psi restated: d = mu - a, rs = 1 / sigma, t = |d rs|, h = exp(-t^2 / 2) (1 / sqrt(2 pi) -
    (t / 2) erfcx(t / sqrt 2)) for t < 40, else 0 (also where t is NaN: sigma = 0 at d = 0), and
    sigma h + max(d, 0).  0 at a = +inf.  mu, sigma: arrays; a: scalar."""
    mu = np.asarray(mu, dtype=np.float64)
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float64), mu.shape)
    if np.isposinf(a):
        return np.zeros(mu.shape)
    with np.errstate(all="ignore"):
        d = mu - a
        rs = 1.0 / sigma
        t = np.abs(d * rs)
        on = t < cutoff
        ts = np.where(on, t, 0.0)
        h = np.where(on, np.exp(-0.5 * (ts * ts)) * (RSQRT2PI - (0.5 * ts) * erfcx(ts * RSQRT2)), 0.0)
        return sigma * h + np.fmax(d, 0.0)


def ehvi_f64(mu, var, boxes, psi=psi_f64):
    """ehvi_direct_value restated: psi at both bounds of every box (0 at +inf), the product left to right
    over the objectives, the sum in box order.  NaN in any row gives NaN."""
    mu = np.asarray(mu, dtype=np.float64)
    var = np.asarray(var, dtype=np.float64)
    m, n = mu.shape
    sigma = np.sqrt(np.abs(var))
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 2 * m)
    cache = {}

    def p(k, a):
        if (k, a) not in cache:
            cache[(k, a)] = np.zeros(n) if np.isposinf(a) else psi(mu[k], sigma[k], a)
        return cache[(k, a)]

    h = np.zeros(n)
    with np.errstate(all="ignore"):
        for b in boxes:
            v = np.ones(n)
            for k in range(m):
                f = p(k, b[k]) - p(k, b[m + k])
                if k < m - 1:
                    v = v * f
                else:
                    h = h + v * f
    return np.where(np.isnan(mu).any(axis=0) | np.isnan(var).any(axis=0), np.nan, h)


def tail_f64(z):
    return 0.5 * special.erfc(z * RSQRT2)


def pof_f64(mu, sigma, lo, hi):
    """ehvi_pof restated: za = (lo - mu) / sigma, zb = (hi - mu) / sigma; Q(za) - Q(zb) for za > 0,
    Q(-zb) - Q(-za) for zb < 0, else (1 - Q(zb)) - Q(-za); sigma = 0 gives 1 inside [lo, hi], else 0."""
    mu = np.asarray(mu, dtype=np.float64)
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float64), mu.shape)
    with np.errstate(all="ignore"):
        za = (lo - mu) / sigma
        zb = (hi - mu) / sigma
        above = za > 0.0
        below = ~above & (zb < 0.0)
        q1 = tail_f64(np.where(above, za, np.where(below, -zb, zb)))
        q2 = tail_f64(np.where(above, zb, -za))
        out = np.where(above | below, q1, 1.0 - q1) - q2
    out = np.where(sigma == 0.0, np.where((lo <= mu) & (mu <= hi), 1.0, 0.0), out)
    return np.where(np.isnan(mu) | np.isnan(sigma), np.nan, out)


def cehvi_f64(mu, var, boxes, bounds, psi=psi_f64, pof=pof_f64):
    """(V, P): fl(E P) with E = ehvi_f64 of the objective rows and P = ((P_0 P_1) P_2) ..., 1 without
    constraints."""
    mu = np.asarray(mu, dtype=np.float64)
    var = np.asarray(var, dtype=np.float64)
    bounds = np.zeros((0, 2)) if bounds is None else np.asarray(bounds, dtype=np.float64).reshape(-1, 2)
    m = mu.shape[0] - bounds.shape[0]
    e = ehvi_f64(mu[:m], var[:m], boxes, psi)
    p = np.ones(mu.shape[1])
    with np.errstate(all="ignore"):
        for j, (lo, hi) in enumerate(bounds):
            pj = pof(mu[m + j], np.sqrt(np.abs(var[m + j])), lo, hi)
            p = pj if j == 0 else p * pj
        return e * p, p

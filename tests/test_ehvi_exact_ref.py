"""tests/ehvi_exact_ref.py against itself and against today's references: the f64 restatement of the device's
arithmetic held to the rounding rule with the recorded C over the sweep, the mpmath statement pinned to
ehvi_ref / cehvi_ref where those keep their digits, the limits, the box maker, and the planted defects: each a
numpy function beside the restatement (no kernel is changed), each caught by the rule -- and (a), (b) and (c)
accepted over the whole sweep by the tolerance the device tests used before it.  No device."""
import functools

import numpy as np
import pytest
from scipy import special

import cehvi_ref as CR
import ehvi_exact_ref as X
import ehvi_ref as ER
import logehvi_ref as LR

INF = np.inf
# z = (mu - edge) / sigma: +60 .. -30, both sides of 0 and of the cutoff t = 40 (t = |z|)
Z_SWEEP = [60.0, 40.1, 40.0, 39.9, 30.0, 10.0, 5.0, 1.0, 0.5, 0.1, 1e-3, 0.0, -1e-3, -0.1, -0.5, -1.0, -2.0, -5.0, -10.0,
           -20.0, -25.0, -29.0, -29.9, -30.0]
ZC_SWEEP = [-30.0, -20.0, -10.0, -5.0, -1.0, -0.1, 0.0, 0.1, 1.0, 5.0, 10.0, 20.0, 30.0]     # the constraints' rows
VARS = [1e-10, 1e-4, 1.0, 25.0]             # sigma^2 from the floor to 25
THIN = 1e-9                                 # two edges this far apart: the kappa case


def sweep_cases():
    """(name, mu, var, boxes, bounds, r): 1 to 4 objectives, sigma^2 from 1e-10 to 25, z from +60 to -30 (less deep
    in the other objectives, so that at most 5 % of a case lies under 2^-900), box pairs whose edges are 1e-9
    apart, sigma = 0 exactly on an edge, and the constraint bands: one-sided each way, two-sided, 1e-6 wide,
    with the mean up to 30 sigma (10 sigma among them) away on either side."""
    rng = np.random.default_rng(11)
    z = np.array(Z_SWEEP)
    cases = []
    for v in VARS:
        s = np.sqrt(v)
        # one objective: the half-open box [0, inf) alone, and cut in two 1e-9 above its lower edge
        mu = (z * s)[None, :]
        var = np.full((1, z.size), v)
        cases.append((f"m=1 var={v}", mu, var, [[0.0, INF]], None, [0.0]))
        cases.append((f"m=1 thin var={v}", mu, var, [[0.0, THIN], [THIN, INF]], None, [0.0]))
        # two objectives: a front with two points 1e-9 apart in the first objective; the z sweep in the first
        # objective against the thin strip's edge, the second objective's z drawn, three draws per z
        front = np.array([[0.5, 0.5], [0.5 + THIN, 0.4], [0.2, 0.8]])
        zz = np.tile(z, 3)
        z2 = rng.uniform(-15.0, 6.0, zz.size)
        mu = np.stack([0.5 + zz * s, 0.5 + z2 * s])
        cases.append((f"m=2 var={v}", mu, np.full(mu.shape, v), LR.boxes_2d(front, [0.0, 0.0]), None, [0.0, 0.0]))
    # 3 and 4 objectives over the m + 1 boxes of a one-point front, sigma mixed per candidate and objective
    for m, deep in ((3, -18.0), (4, -15.0)):
        n = 48
        f = np.full(m, 0.5)
        sg = np.sqrt(rng.choice(VARS, (m, n)))
        zz = rng.uniform(deep, 6.0, (m, n))
        zz[0, :z.size] = np.maximum(z, deep)              # the first objective walks the sweep as far as `deep`
        zz[1, :4] = 60.0
        cases.append((f"m={m}", f[:, None] + zz * sg, sg * sg, X.boxes_one_point(f, np.zeros(m)), None, np.zeros(m)))
    # sigma = 0: on an edge, between edges, below and above all of them; in both objectives and in one
    front = np.array([[0.5, 0.5], [0.2, 0.8]])
    mu0 = np.array([0.5, 0.2, 0.0, 0.3, -1.0, 2.0, 0.5, 0.2])
    mu = np.stack([mu0, np.array([0.5, 0.8, 0.6, 0.0, 0.7, 0.9, 0.7, 0.1])])
    var = np.zeros(mu.shape)
    var[1, 6:] = 0.25
    cases.append(("sigma=0", mu, var, LR.boxes_2d(front, [0.0, 0.0]), None, [0.0, 0.0]))
    # constraints: one objective of moderate EHVI, the constraint's mean from 30 sigma under to 30 sigma over
    # the band; then pairs of constraints, the second one's z drawn within 5
    zc = np.array(ZC_SWEEP)
    for v in VARS:
        s = np.sqrt(v)
        obj_mu, obj_var = np.full((1, zc.size), 0.3), np.full((1, zc.size), 0.04)
        bands = {"lower": (0.5, INF), "upper": (-INF, 0.5), "two-sided": (0.5 - 3.0 * s, 0.5 + 2.0 * s),
                 "1e-6 wide": (0.5, 0.5 + 1e-6)}
        for name, (lo, hi) in bands.items():
            row = (lo if np.isfinite(lo) else hi) + zc * s
            mu = np.concatenate([obj_mu, row[None, :]])
            var = np.concatenate([obj_var, np.full((1, zc.size), v)])
            cases.append((f"{name} var={v}", mu, var, [[0.0, INF]], [[lo, hi]], [0.0]))
            row2 = 0.1 + rng.uniform(-5.0, 5.0, zc.size) * s
            cases.append((f"{name} and another var={v}", np.concatenate([mu, row2[None, :]]),
                          np.concatenate([var, np.full((1, zc.size), v)]), [[0.0, INF]], [[lo, hi], [0.1, INF]], [0.0]))
    return cases


@functools.lru_cache(maxsize=None)
def sweep():
    out = []
    for name, mu, var, boxes, bounds, r in sweep_cases():
        rules = X.reference(mu, var, boxes, bounds)
        out.append((name, mu, var, np.asarray(boxes, dtype=np.float64), bounds, np.asarray(r, dtype=np.float64), rules))
    return out


def test_every_case_qualifies():
    """On the reference alone: every F_bk <= 2^10, and at most 5 % of a case's candidates under 2^-900."""
    for name, mu, var, boxes, bounds, r, (e, p, v) in sweep():
        assert e.qualifies() and v.qualifies(), (name, e.fmax, e.low.mean(), v.low.mean())
    assert sum(int(e.held.sum()) for *_, (e, p, v) in sweep()) > 500


def test_restatement_meets_the_rule_with_the_recorded_c():
    """C_RULE is the smallest power of two >= twice the worst measured (err / u - base)+ / k of the restatement,
    over E, pof_out and V."""
    worst = {"E": 0.0, "P": 0.0, "V": 0.0}
    for name, mu, var, boxes, bounds, r, (e, p, v) in sweep():
        got_v, got_p = X.cehvi_f64(mu, var, boxes, bounds)
        m = mu.shape[0] - (0 if bounds is None else len(bounds))
        got_e = X.ehvi_f64(mu[:m], var[:m], boxes)
        ce, cp, cv = e.c_needed(got_e), p.c_needed(got_p), v.c_needed(got_v)
        print(f"{name}: C needed by E {ce:.3g}, pof {cp:.3g}, V {cv:.3g}")
        worst = {"E": max(worst["E"], ce), "P": max(worst["P"], cp), "V": max(worst["V"], cv)}
        for rule, got in ((e, got_e), (p, got_p), (v, got_v)):
            assert rule.check(got)[0] == 0, name
    print(f"worst measured C: {worst}; recorded {X.C_MEASURED}, rule {X.C_RULE}")
    assert max(worst.values()) <= X.C_MEASURED
    assert X.C_RULE >= 2 * X.C_MEASURED and X.C_RULE / 2 < 2 * X.C_MEASURED
    assert X.C_RULE == 2.0 ** round(np.log2(X.C_RULE))


def test_reference_agrees_with_todays_references():
    """Where z >= -4 in every objective (test_gpu_ehvi.test_empty_front's range: phi + z Phi keeps its digits)
    ehvi_ref.ehvi is the mpmath value to rel 1e-11 (thin boxes: to 1e-11 of the box sum's scale); and
    cehvi_ref's P to 1e-9 relative plus 1e-15 (its central branch rounds 1 - Q) where P >= 1e-12."""
    seen = 0
    for name, mu, var, boxes, bounds, r, (e, p, v) in sweep():
        m = len(r)
        with np.errstate(all="ignore"):
            z = (mu[:m] - boxes[:, :m].min(axis=0)[:, None]) / np.sqrt(np.abs(var[:m]))
            ok = e.held & (z >= -4.0).all(axis=0)
        lin = ER.ehvi(mu[:m], var[:m], boxes)
        seen += int(ok.sum())
        assert (np.abs(lin[ok] - e.val[ok]) <= 1e-11 * ER.scale(mu[:m, ok], var[:m, ok], r)).all(), name
        if bounds is not None:
            pr = CR.pof_product(mu[m:], var[m:], np.asarray(bounds))
            okp = p.held & (p.val >= 1e-12)
            assert np.allclose(pr[okp], p.val[okp], rtol=1e-9, atol=1e-15), name
    assert seen > 200


def test_limits_and_underflow():
    one = [[0.0, INF]]
    # sigma = 0: psi(a) = max(mu - a, 0) exactly; E = 0 at and below the edge, with bound 0
    e, _, _ = X.reference(np.array([[2.0, 0.0, -1.0]]), np.zeros((1, 3)), one)
    assert e.val.tolist() == [2.0, 0.0, 0.0] and e.zero.tolist() == [False, True, True] and e.bound[1] == 0.0
    assert e.check(np.array([2.0, 0.0, 0.0])) == (0, 0.0)
    assert e.check(np.array([2.0, 1e-300, 0.0]))[0] == 1 and e.check(np.array([2.0, np.nan, 0.0]))[0] == 1
    # no box: 0 everywhere; NaN in any objective row: NaN, and P keeps its value; NaN in a constraint row: V and P
    e, _, _ = X.reference(np.array([[0.5]]), np.array([[1.0]]), np.zeros((0, 2)))
    assert e.zero.all()
    mu, var = np.array([[0.5, np.nan, 0.5, 0.5], [0.2, 0.2, 0.2, np.nan]]), np.array([[1.0, 1.0, np.nan, 1.0], [1.0] * 4])
    e, p, v = X.reference(mu, var, one, [[0.0, INF]])
    assert e.nan.tolist() == [False, True, True, False] and p.nan.tolist() == [False, False, False, True]
    assert v.nan.tolist() == [False, True, True, True]
    got_v, got_p = X.cehvi_f64(mu, var, one, [[0.0, INF]])
    assert np.array_equal(np.isnan(got_v), v.nan) and np.array_equal(np.isnan(got_p), p.nan)
    assert v.check(got_v)[0] == 0 and v.check(np.where(v.nan, 0.0, got_v))[0] == 3
    # (-inf, +inf) is exactly 1 and sigma = 0 outside the band exactly 0; a negative var is sigma = sqrt(|var|)
    e, p, v = X.reference(np.array([[0.5, 0.5], [3.0, 3.0]]), np.array([[-1.0, 1.0], [4.0, 0.0]]), one, [[-INF, INF]])
    assert p.val.tolist() == [1.0, 1.0] and e.ref[0] == e.ref[1] == v.ref[0]
    _, p, v = X.reference(np.array([[0.5], [3.0]]), np.array([[1.0], [0.0]]), one, [[0.0, 1.0]])
    assert p.zero.all() and v.zero.all() and v.bound[0] == 0.0
    # underflow: z = -45 is 1e-443, under 2^-900: any value in [0, 2^-899] is accepted, nothing else
    e, _, _ = X.reference(np.array([[-45.0, -30.0]]), np.ones((1, 2)), one)
    assert e.low.tolist() == [True, False] and not e.qualifies()
    good = X.ehvi_f64(np.array([[-45.0, -30.0]]), np.ones((1, 2)), one)
    assert good[0] == 0.0 and e.check(good)[0] == 0 and e.check(np.array([2.0 ** -899, good[1]]))[0] == 0
    assert e.check(np.array([2.0 ** -898, good[1]]))[0] == 1 and e.check(np.array([-0.0, 0.0]))[0] == 1
    # F_bk > 2^10 disqualifies a case
    assert not X.reference(np.array([[2000.0]]), np.ones((1, 1)), one)[0].qualifies()


@pytest.mark.parametrize("m", [2, 3, 4])
def test_boxes_one_point_is_a_partition(m):
    rng = np.random.default_rng(m)
    f, r = rng.uniform(0.3, 0.7, m), np.zeros(m)
    boxes = X.boxes_one_point(f, r)
    assert boxes.shape == (m + 1, 2 * m)
    pts = rng.uniform(0.0, 1.0, (4000, m))
    inside = ((pts[:, None, :] >= boxes[None, :, :m]) & (pts[:, None, :] < boxes[None, :, m:])).all(-1)
    dominated = (pts <= f).all(-1)
    assert ((inside.sum(1) == 1) == ~dominated).all() and (inside.sum(1) <= 1).all()
    assert all(np.isfinite(boxes[:, m + k]).any() for k in range(m))


# ------------------------------------------------------------------------------- the planted defects
def _phi_difference(mu, sigma, lo, hi):
    """(f): P as Phi(zb) - Phi(za), Phi(z) = erfc(-z / sqrt 2) / 2."""
    with np.errstate(all="ignore"):
        za, zb = (lo - mu) / sigma, (hi - mu) / sigma
        out = 0.5 * special.erfc(-zb * X.RSQRT2) - 0.5 * special.erfc(-za * X.RSQRT2)
    return np.where(sigma == 0.0, np.where((lo <= mu) & (mu <= hi), 1.0, 0.0), out)


def _swapped(boxes):
    """(e): l and u of the first objective swapped in the first box that has both finite."""
    b = np.array(boxes, dtype=np.float64)
    m = b.shape[1] // 2
    rows = np.flatnonzero(np.isfinite(b[:, m]))
    if rows.size:
        i = rows[0]
        b[i, 0], b[i, m] = b[i, m], b[i, 0]
    return b


DEFECTS = {
    "a": dict(psi=ER.psi),
    "b": dict(psi=functools.partial(X.psi_f64, erfcx=lambda x: special.erfcx(x) * (1.0 + 1e-12))),
    "c": dict(psi=functools.partial(X.psi_f64, cutoff=30.0)),
    "d": dict(boxes=lambda b: b[:-1]),
    "e": dict(boxes=_swapped),
    "f": dict(pof=_phi_difference),
}
TODAY_PASSES = ("a", "b", "c")


def _today(mu, var, r, p, v, got_v):
    """Per candidate without NaN: |value - E_ref P_ref| <= HVI_RTOL (prod_k psi_k(r_k) + 1) P_ref, the tolerance of
    tests/test_gpu_ehvi.py's _close, times P as tests/test_gpu_cehvi.py's selection and loop tests apply it."""
    m = len(r)
    fin = ~v.nan
    tol = ER.HVI_RTOL * ER.scale(mu[:m, fin], var[:m, fin], r) * np.where(p.nan[fin], 1.0, p.val[fin])
    with np.errstate(all="ignore"):
        return np.abs(got_v[fin] - v.val[fin]) <= tol


def _defect_run(name):
    """Over the sweep: (candidates that miss the new rule, candidates that miss today's tolerance, candidates
    left out of the latter).  Left out are the candidates at which the restatement ITSELF misses today's
    tolerance: a band 1e-6 wide under sigma = 5 with the mean 20 sigma and more away, where P = Q(za) - Q(zb)
    keeps 1e-8 of its digits at best.  Today's tests have no such candidate -- the device would miss there."""
    d = DEFECTS[name]
    missed = today_missed = left_out = 0
    for case, mu, var, boxes, bounds, r, (e, p, v) in sweep():
        if "pof" in d and bounds is None:
            continue
        bx = d["boxes"](boxes) if "boxes" in d else boxes
        got_v, got_p = X.cehvi_f64(mu, var, bx, bounds, psi=d.get("psi", X.psi_f64), pof=d.get("pof", X.pof_f64))
        missed += v.check(got_v)[0] + p.check(got_p)[0]
        base = _today(mu, var, r, p, v, X.cehvi_f64(mu, var, boxes, bounds)[0])
        left_out += int((~base).sum())
        today_missed += int((base & ~_today(mu, var, r, p, v, got_v)).sum())
    return missed, today_missed, left_out


@pytest.mark.parametrize("name", sorted(DEFECTS))
def test_planted_defect(name):
    """The rule fails on the sweep for every defect.  Today's tolerance passes the whole sweep for (a), (b) and
    (c): the record of the gap.  It does NOT pass (f): Phi(zb) - Phi(za) is wrong where the band lies above the
    mean (1 - 1 = 0 from 8.3 sigma on), and there an error of E P_ref against a tolerance of 1e-9 scale P_ref is
    not hidden; tests/test_gpu_cehvi.py's own bound on pof_out (2 (8 z^2 + 32) u T) finds it as well.  (d) and
    (e) move the value by whole terms and were never in the gap."""
    missed, today_missed, left_out = _defect_run(name)
    print(f"defect ({name}): {missed} candidates miss the rule; {today_missed} miss today's tolerance ({left_out} left out)")
    assert missed > 0
    assert left_out <= 6
    if name in TODAY_PASSES:
        assert today_missed == 0
    else:
        assert today_missed > 0

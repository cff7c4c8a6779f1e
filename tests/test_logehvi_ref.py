"""tests/logehvi_ref.py against itself and against the linear references: the mpmath statement pinned
to log(ehvi_ref.ehvi) / log(cehvi_ref.cehvi) where those are well above their underflow, the f64
restatement of the device's arithmetic held to the rounding rule with the recorded C over the sweep,
the limits, the admission-rule mirror and the motivating case (reference only).  No device."""
import numpy as np
import pytest

import cehvi_ref as CR
import ehvi_ref as ER
import logehvi_ref as R

INF = np.inf
Z_SWEEP = [8.0, 6.1, 6.0, 5.9, 4.0, 1.0, 0.5, 0.1, 1e-3, 0.0, -1e-3, -0.1, -0.5, -1.0, -5.0, -5.9, -6.0, -6.1, -10.0,
           -31.9, -32.0, -32.1, -39.9, -40.0, -40.1, -100.0, -1e3, -1e4, -1e5, -1e6]
SIGMAS = [1e-5, 1e-3, 1.0, 1e3]


def sweep_cases():
    """(name, mu, var, boxes, bounds): z from +8 to -1e6 and on both sides of each branch switch (0, 6, 32, 40), sigma from
    1e-5 to 1e3, thin and wide boxes, 1 to 4 objectives, 0, 1 and 7 constraints."""
    rng = np.random.default_rng(5)
    cases = []
    z = np.array(Z_SWEEP)
    for s in SIGMAS:
        # one objective, one half-open box [l, inf): L = ln psi(l)
        l = 0.75
        cases.append((f"z-sweep sigma={s}", (l + z * s)[None, :], np.full((1, z.size), s * s), [[l, INF]], None))
        # two objectives, a thin and a wide closed box and a half-open one; the second objective's z drawn
        mu = np.stack([l + z * s, 0.3 + rng.uniform(-6.0, 3.0, z.size) * s])
        boxes = [[l, 0.3, l + 1e-6 * s, 0.3 + 2.0 * s], [l + 1e-6 * s, 0.3, l + 50.0 * s, INF],
                 [l + 50.0 * s, 0.3 + 2.0 * s, INF, INF]]
        cases.append((f"thin/wide sigma={s}", mu, np.full((2, z.size), s * s), boxes, None))
    # 3 and 4 objectives over random boxes sharing edges, sigma mixed per candidate
    for m in (3, 4):
        n = 24
        edges = np.sort(rng.uniform(-1.0, 1.0, (m, 4)), axis=1)
        boxes = []
        for _ in range(7):
            lo = rng.integers(0, 3, m)
            hi = lo + 1 + rng.integers(0, 2, m)
            boxes.append([edges[k, lo[k]] for k in range(m)] + [edges[k, hi[k]] if hi[k] < 4 else INF for k in range(m)])
        sg = 10.0 ** rng.uniform(-5.0, 3.0, (m, n))
        mu = rng.uniform(-1.0, 1.0, (m, n)) + sg * rng.uniform(-30.0, 4.0, (m, n))
        cases.append((f"{m} objectives", mu, sg * sg, boxes, None))
    # constraints: one-sided, two-sided (thin and wide), (-inf, +inf); z over the sweep
    for s in SIGMAS:
        mu_o = np.full((1, z.size), 0.1)
        rows = [0.5 + z * s, 0.5 - z * s, 0.5 + z * s, 0.5 + z * s, 0.5 + 0.1 * z * s, rng.uniform(-1, 1, z.size),
                0.5 - 0.3 * z * s]
        bounds = [[0.5, INF], [-INF, 0.5], [0.5, 0.5 + 1e-6 * s], [0.5 - 3.0 * s, 0.5 + 2.0 * s], [-INF, 0.5],
                  [-INF, INF], [0.5, 0.5 + 5.0 * s]]
        mu = np.concatenate([mu_o, np.stack(rows)])
        var = np.concatenate([np.full((1, z.size), 0.04), np.full((7, z.size), s * s)])
        cases.append((f"7 constraints sigma={s}", mu, var, [[0.0, INF]], bounds))
        cases.append((f"1 constraint sigma={s}", mu[:2], var[:2], [[0.0, INF]], bounds[:1]))
        # seven tails of like size: the chain of six additions of logarithms of one sign
        zz = rng.uniform(0.7, 1.3, (7, z.size)) * np.minimum(z, -0.5)
        cases.append((f"7 like constraints sigma={s}", np.concatenate([mu_o, 0.5 + zz * s]), var, [[0.0, INF]],
                      [[0.5, INF]] * 7))
    return cases


@pytest.fixture(scope="module")
def sweep():
    out = []
    for name, mu, var, boxes, bounds in sweep_cases():
        ref = R.reference(mu, var, boxes, bounds, c=1.0)
        out.append((name, mu, var, np.asarray(boxes, dtype=np.float64), bounds, ref))
    return out


def test_restatement_meets_the_rule_with_the_recorded_c(sweep):
    """C_RULE is the smallest power of two >= twice the worst measured (err / u - n_boxes - 2)+ / K."""
    worst, worst_lp = 0.0, 0.0
    for name, mu, var, boxes, bounds, (lref, b1, lpref, lpb1) in sweep:
        got, lp = R.logehvi_f64(mu, var, boxes, bounds)
        nb = boxes.shape[0]
        fin = np.isfinite(lref)
        assert np.array_equal(got[~fin], lref[~fin], equal_nan=True), name
        k = b1[fin] / R.U - nb - 2
        extra = np.maximum(np.abs(got[fin] - lref[fin]) / R.U - nb - 2, 0.0)
        with np.errstate(all="ignore"):
            r = np.where(extra > 0, extra / k, 0.0)
        finp = np.isfinite(lpref)
        assert np.array_equal(lp[~finp], lpref[~finp], equal_nan=True), name
        kp = lpb1[finp] / R.U - 2
        ep = np.maximum(np.abs(lp[finp] - lpref[finp]) / R.U - 2, 0.0)
        with np.errstate(all="ignore"):
            rp = np.where(ep > 0, ep / kp, 0.0)
        print(f"{name}: worst C {r.max() if r.size else 0:.3g}, logpof {rp.max() if rp.size else 0:.3g}")
        worst, worst_lp = max(worst, r.max() if r.size else 0.0), max(worst_lp, rp.max() if rp.size else 0.0)
    print(f"worst measured C {worst:.4g} (logpof alone {worst_lp:.4g}); recorded {R.C_MEASURED}, rule {R.C_RULE}")
    assert max(worst, worst_lp) <= R.C_MEASURED
    assert R.C_RULE >= 2 * R.C_MEASURED and R.C_RULE / 2 < 2 * R.C_MEASURED
    assert R.C_RULE == 2.0 ** round(np.log2(R.C_RULE))


def test_reference_is_log_of_the_linear_references(sweep):
    """Wherever ehvi_ref.ehvi / cehvi_ref.cehvi are above 2^-500 the mpmath L is their logarithm, to the
    linear references' own accuracy (HVI_RTOL on the box sum's scale, cancellation in phi + z Phi)."""
    seen = 0
    for name, mu, var, boxes, bounds, (lref, _, _, _) in sweep:
        lin = ER.ehvi(mu, var, boxes) if bounds is None else CR.cehvi(mu, var, boxes, bounds)
        m = mu.shape[0] - (0 if bounds is None else len(bounds))
        z = (mu[:m] - np.min(boxes[:, :m], axis=0)[:, None]) / np.sqrt(np.abs(var[:m]))
        ok = (lin > 2.0 ** -500) & (z > -6.0).all(axis=0)        # phi + z Phi keeps 1e-16 z^2 e^(z^2/2)-ish
        seen += int(ok.sum())
        assert np.allclose(lref[ok], np.log(lin[ok]), rtol=0, atol=1e-6), name
    assert seen > 100


def test_limits():
    inf = INF
    one = [[0.0, inf]]
    # sigma = 0: psi(a) = max(mu - a, 0); L = ln(mu - a), or -inf at and below the bound
    mu = np.array([[2.0, 0.0, -1.0]])
    for f in (lambda *a: R.reference(*a)[0], lambda *a: R.logehvi_f64(*a)[0]):
        got = f(mu, np.zeros((1, 3)), one, None)
        assert got[0] == pytest.approx(np.log(2.0), abs=1e-15) and got[1] == -inf and got[2] == -inf
        # a box with a zero factor contributes nothing; no box at all gives -inf
        two = [[0.0, 0.0, 1.0, inf], [1.0, 5.0, inf, inf]]
        got = f(np.array([[0.5], [3.0]]), np.zeros((2, 1)), two, None)
        assert got[0] == pytest.approx(np.log(0.5 * 3.0), abs=1e-15)
        assert f(np.array([[0.5]]), np.array([[1.0]]), np.zeros((0, 2)), None)[0] == -inf
        # P_j = 0 (sigma = 0 outside the bounds) gives -inf; (-inf, +inf) adds exactly 0
        mu2, var2 = np.array([[0.5, 0.5], [3.0, 3.0]]), np.array([[1.0, 1.0], [0.0, 4.0]])
        assert f(mu2, var2, one, [[0.0, 1.0]])[0] == -inf
        a = f(mu2, var2, one, [[-inf, inf]])
        b = f(mu2[:1], var2[:1], one, None)
        assert np.array_equal(a, b)
        # NaN in any row, objective or constraint, mean or variance
        for r, arr in ((0, "mu"), (1, "mu"), (0, "var"), (1, "var")):
            m3, v3 = mu2.copy(), var2.copy()
            (m3 if arr == "mu" else v3)[r, 1] = np.nan
            got = f(m3, v3, one, [[0.0, 4.0]])
            assert np.isnan(got[1]) and not np.isnan(got[0])


def test_finite_and_ordered_far_below_the_front():
    """z down to -1e6: the linear value is 0.0 from z = -40 on, the log value finite and decreasing."""
    z = np.array([-10.0, -38.0, -40.0, -100.0, -1e3, -1e6])
    mu, var = z[None, :], np.ones((1, z.size))
    lin = ER.ehvi(mu, var, [[0.0, INF]])
    assert (lin[2:] == 0.0).all() or lin[3] == 0.0
    for got in (R.reference(mu, var, [[0.0, INF]])[0], R.logehvi_f64(mu, var, [[0.0, INF]])[0]):
        assert np.isfinite(got).all() and (np.diff(got) < 0).all()
        assert got[-1] == pytest.approx(-0.5e12 - np.log(np.sqrt(2 * np.pi)) - 2 * np.log(1e6), rel=1e-12)


def test_table_threads_mirror():
    assert [R.table_threads(s) for s in (0, 40, 41, 80, 81, 160, 161)] == [256, 256, 128, 128, 64, 64, 0]
    assert R.table_threads(-1) == 0
    assert all(R.table_threads(s) in (0,) + R.TABLE_THREADS for s in range(0, 400))
    assert all(R.table_threads(s) == 0 or 16 * s * R.table_threads(s) <= R.LDS_BYTES for s in range(0, 400))


def test_boxes_2d_is_a_partition():
    rng = np.random.default_rng(0)
    a = np.sort(rng.uniform(0, 1, 6))
    front = np.stack([a, 1.0 - a], 1)
    boxes = R.boxes_2d(front, [-0.1, -0.1])
    pts = rng.uniform(-0.1, 1.5, (2000, 2))
    inside = ((pts[:, None, :] >= boxes[None, :, :2]) & (pts[:, None, :] < boxes[None, :, 2:])).all(-1)
    dominated = (front[None, :, :] >= pts[:, None, :]).all(-1).any(-1)
    assert ((inside.sum(1) == 1) == ~dominated).all() and (inside.sum(1) <= 1).all()


@pytest.fixture(scope="module")
def motivating():
    c = R.motivating_case()
    boxes = R.boxes_2d(c["front"], c["ref_point"])
    lref, bound, _, _ = R.reference(c["mu"], c["var"], boxes)
    return c, boxes, lref, bound


def test_motivating_case_on_the_reference(motivating):
    """N = 120, one length scale of 200 on the 33 x 31 grid: the linear EHVI is exactly 0 at >= 95 % of the
    unevaluated candidates and positive at fewer than 16, so its top-16 runs into index order; the log value is
    finite everywhere and its top 17 are separated by more than twice the rule's bound."""
    c, boxes, lref, bound = motivating
    free = ~c["evaluated"]
    lin = ER.ehvi(c["mu"], c["var"], boxes)
    share0 = float((lin[free] == 0.0).mean())
    pos = int((lin[free] > 0.0).sum())
    picks, gaps, nxt = R.select_top(lref, c["evaluated"], 17)
    tol = np.maximum(bound[picks], bound[nxt])
    print(f"share of exact zeros {share0:.4f}, positive {pos}, L in [{lref.min():.6g}, {lref.max():.6g}], "
          f"distinct among free {np.unique(lref[free]).size} of {free.sum()}, min top-17 gap {gaps[:16].min():.4g}, "
          f"max bound {tol.max():.3g}; picks {picks[:16].tolist()}")
    assert share0 >= 0.95 and 0 < pos < 16
    assert np.isfinite(lref).all()
    assert (gaps[:16] > 2 * tol[:16]).all()
    # the linear order agrees with the log order on its positive candidates, then falls back to the index order
    lin_picks, _, _ = R.select_top(lin, c["evaluated"], 16)
    assert lin_picks[:pos].tolist() == picks[:pos].tolist()
    assert lin_picks[pos:].tolist() == np.flatnonzero(free & (lin == 0.0))[:16 - pos].tolist()
    assert lin_picks[pos:].tolist() != picks[pos:16].tolist()
    # and the restatement meets the rule here too
    got, _ = R.logehvi_f64(c["mu"], c["var"], boxes)
    out, worst = R.check_rule(got, lref, bound)
    print(f"restatement: share outside the rule {out}, worst fraction of the bound {worst:.3g}")
    assert out == 0.0

"""The EHVI and the constrained EHVI on the device (bo_expected_hypervolume_improvement, bo_constrained_ehvi,
the scan inside bo_select_batch_kb and ehvi_select_indices; direct and table forms) against the mpmath
statement of tests/ehvi_exact_ref.py.  PARITY UNPINNED by the reference, which has no EHVI.

Every value is held to the rounding rule at EVERY candidate, however small the value:
    |E - E_ref|       <= bound_E = u [C Kbox + (n_boxes + n_obj + 1) E_ref],   C = 16, u = 2^-53
    |V - E_ref P_ref| <= P_ref bound_E + E_ref P_ref u [C Kcon + n_con + 1]    (pof_out: the second term / E_ref)
NaN and an exact 0 of the reference are met exactly; a reference under 2^-900 asks for a value in [0, 2^-899].
Every case asserts ON THE REFERENCE ALONE that all F_bk <= 2^10 and that at most 5 % of its candidates lie
under 2^-900 (the two cases exempt say so).  mu and var are built on the host and uploaded; the mpmath
references are computed once per case and shared.  The device's worst fraction of the bound over this file:
see DESIGN.md section 11."""
import functools

import numpy as np
import pytest

import ehvi_exact_ref as X
import logehvi_ref as LR
from test_gpu_cehvi import KINDS, _constraint_rows
from test_gpu_cehvi import _scan as _cscan
from test_gpu_ehvi import REF, _posterior, _staircase
from test_hvi import _front

pytestmark = pytest.mark.gpu

FORMS = ("direct", "table", "auto")
INF = np.inf
CAP = {1: 1500, 2: 1500, 3: 800, 4: 400}           # candidates per case: its mpmath reference takes under 10 s
DEPTH = {1: 30.0, 2: 21.0, 3: 17.0, 4: 14.5}        # the deepest z per objective of the candidates pushed under


@pytest.fixture(scope="module")
def bo():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import bayesopt_smart_amd as bo
    return bo


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64))


def _push_under(rng, mu, var, boxes, r, depth):
    """Every third candidate from column 12 on goes 5 .. depth standard deviations under the lowest edge of
    every objective (the reference point's coordinate, or the lowest front coordinate the boxes start from):
    where a fitted loop's candidates sit, and where the value is far below 1e-9."""
    m, n = mu.shape
    cols = np.arange(12, n)[2::3]
    low = boxes[:, :m].min(axis=0) if boxes.shape[0] else np.asarray(r, dtype=np.float64)
    z = rng.uniform(5.0, depth, (m, cols.size))
    mu[:, cols] = low[:, None] - z * np.sqrt(var[:, cols])
    return cols


@functools.lru_cache(maxsize=None)
def _case(m, kind, p):
    """test_gpu_ehvi's front (m, kind, p) and special columns, CAP[m] candidates, a third of them pushed under
    the front: (front, r, boxes, mu, var)."""
    from bayesopt_smart_amd.acquisition import hypervolume_boxes
    rng = np.random.default_rng(31 * m + p + (kind == "int"))
    front = _front(rng, p, m, kind)
    r = np.full(m, REF)
    boxes = hypervolume_boxes(front, r)
    mu, var = _posterior(rng, m, CAP[m], front)
    _push_under(rng, mu, var, boxes, r, DEPTH[m])
    for a in (front, r, boxes, mu, var):
        a.setflags(write=False)
    return front, r, boxes, mu, var


@functools.lru_cache(maxsize=None)
def _box(m, kind, p):
    """The mpmath box part of _case, computed once and shared by the plain and the constrained tests."""
    front, r, boxes, mu, var = _case(m, kind, p)
    return X.box_part(mu, var, boxes)


@functools.lru_cache(maxsize=None)
def _rule(m, kind, p):
    e = X.combine(_box(m, kind, p), [], _case(m, kind, p)[2].shape[0], m)[0]
    assert e.qualifies(), (e.fmax, e.low.mean())                      # on the reference alone
    tiny = e.held & (e.val < 1e-9)
    assert tiny.mean() > 0.2 and e.nan.sum() >= 2                      # the values no test looked at before
    return e


def _ehvi(mu_d, var_d, tables, form):
    from bayesopt_smart_amd.acquisition import expected_hypervolume_improvement
    return expected_hypervolume_improvement(mu_d, var_d, None, None, form=form, tables=tables).cpu().numpy()


@pytest.mark.parametrize("p", [12, 17])
@pytest.mark.parametrize("kind", ["int", "cont"])
@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_rule_at_every_candidate(bo, m, kind, p):
    """n in {1, 255, 257, CAP[m]} x the three forms: the rule at every candidate, the limits exactly, and the
    table form and auto equal to the direct form bit for bit."""
    import torch
    from bayesopt_smart_amd.acquisition import EhviTables
    front, r, boxes, mu, var = _case(m, kind, p)
    rule = _rule(m, kind, p)
    tables = EhviTables(front, r, "cuda")
    assert tables.threads > 0 and tables.n_boxes == boxes.shape[0]
    worst = 0.0
    for n in (1, 255, 257, CAP[m]):
        mu_d = torch.tensor(mu[:, :n], device="cuda")                  # copies: the case is shared
        var_d = torch.tensor(var[:, :n], device="cuda")
        got = {f: _ehvi(mu_d, var_d, tables, f) for f in FORMS}
        head = rule.head(n)
        for f in FORMS:
            miss, w = head.check(got[f])
            worst = max(worst, w)
            assert miss == 0, (f, n, miss, w)
        assert same_bits(got["table"], got["direct"]) and same_bits(got["auto"], got["direct"])
    print(f"m={m} {kind} p={p}: {boxes.shape[0]} boxes, {int(rule.held.sum())} candidates under the rule "
          f"({int((rule.held & (rule.val < 1e-9)).sum())} of them below 1e-9, {int(rule.low.sum())} under 2^-900): "
          f"worst |E - E_ref| / bound = {worst:.3g}")


TABLE_SUMS = (80, 160, 320, 400)                    # sum_k E_k: the largest of T = 256, 128, 64, and no table


def _stair_n(s):
    """300 candidates, fewer where 300 would take the reference past 10 s (it costs candidates x edges)."""
    return min(300, 40000 // s)


@functools.lru_cache(maxsize=None)
def _stair(s):
    from bayesopt_smart_amd.acquisition import hypervolume_boxes
    rng = np.random.default_rng(9 + s)
    front, r = _staircase(s // 2 - 1), np.full(2, REF)
    boxes = hypervolume_boxes(front, r)
    mu, var = _posterior(rng, 2, _stair_n(s), front)
    _push_under(rng, mu, var, boxes, r, DEPTH[2])
    rule = X.reference(mu, var, boxes)[0]
    assert rule.qualifies(), (rule.fmax, rule.low.mean())
    return front, r, boxes, mu, var, rule


@pytest.mark.parametrize("s", TABLE_SUMS)
def test_table_workgroup_sizes(bo, s):
    """test_gpu_ehvi.test_admission_thresholds' staircase fronts at the largest sum_k E_k of each workgroup size
    of the table form and one past every table: the rule in place of that test's tolerance."""
    import torch
    import ehvi_ref as ER
    from bayesopt_smart_amd.acquisition import EhviTables
    front, r, boxes, mu, var, rule = _stair(s)
    tables = EhviTables(front, r, "cuda")
    want_t = {80: 256, 160: 128, 320: 64, 400: 0}[s]
    assert tables.sum_edges == s and tables.threads == want_t == ER.table_threads(s)
    mu_d, var_d = torch.tensor(mu, device="cuda"), torch.tensor(var, device="cuda")
    auto = _ehvi(mu_d, var_d, tables, "auto")
    miss, worst = rule.check(auto)
    print(f"sum_edges={s} T={want_t} n={mu.shape[1]}: worst |E - E_ref| / bound = {worst:.3g}")
    assert miss == 0, (miss, worst)
    assert same_bits(_ehvi(mu_d, var_d, tables, "direct"), auto)
    if want_t:
        assert same_bits(_ehvi(mu_d, var_d, tables, "table"), auto)


@functools.lru_cache(maxsize=None)
def _motivating():
    from bayesopt_smart_amd.acquisition import hypervolume_boxes
    c = LR.motivating_case()
    boxes = hypervolume_boxes(c["front"], c["ref_point"])
    rule = X.reference(c["mu"], c["var"], boxes)[0]
    lref, lbound, _, _ = LR.reference(c["mu"], c["var"], boxes)
    return c, boxes, rule, lref, lbound


def test_motivating_case(bo):
    """logehvi_ref.motivating_case(): 1023 candidates of a fitted loop.  EXEMPT from the 5 % cap, underflow being
    its point: the share under 2^-900 is printed and every such candidate must lie in [0, 2^-899]; the others meet
    the rule.  And where "ehvi" is under the rule and "logehvi" finite, |log(ehvi) - logehvi| is within the sum of
    the two rules' bounds (the linear one carried to the logarithm: -log1p(-bound / E_ref))."""
    import torch
    from bayesopt_smart_amd.acquisition import EhviTables, log_expected_hypervolume_improvement
    c, boxes, rule, lref, lbound = _motivating()
    assert rule.fmax <= X.F_MAX and not rule.nan.any()
    tables = EhviTables(c["front"], c["ref_point"], "cuda")
    mu_d, var_d = torch.tensor(c["mu"], device="cuda"), torch.tensor(c["var"], device="cuda")
    got = _ehvi(mu_d, var_d, tables, "direct")
    miss, worst = rule.check(got)
    print(f"motivating case: {boxes.shape[0]} boxes; {rule.low.mean():.4f} of the candidates under 2^-900 (left to the "
          f"range check), {int(rule.held.sum())} under the rule, {int((rule.held & (rule.val < 1e-9)).sum())} of them below "
          f"1e-9; worst |E - E_ref| / bound = {worst:.3g}")
    assert miss == 0 and rule.held.sum() >= 5
    if tables.threads:
        assert same_bits(_ehvi(mu_d, var_d, tables, "table"), got)
    log = log_expected_hypervolume_improvement(mu_d, var_d, None, None, form="direct", tables=tables).cpu().numpy()
    both = rule.held & np.isfinite(log) & (got > 0.0)
    assert both.sum() == rule.held.sum()
    with np.errstate(all="ignore"):
        allow = -np.log1p(-rule.bound[both] / rule.val[both]) + lbound[both]
        diff = np.abs(np.log(got[both]) - log[both])
    print(f"|log(ehvi) - logehvi| / (the two bounds) at {int(both.sum())} candidates: worst {float((diff / allow).max()):.3g}")
    assert (diff <= allow).all()


TAIL_N, TAIL_Q = 1024, 16
TAIL_EVALUATED = np.array([0, 5, 17, 100, 101, 640, 1023])


@functools.lru_cache(maxsize=None)
def _tail():
    """2 objectives, 1024 candidates 7 .. 20 standard deviations under the reference point in both: every EHVI
    in [1e-200, 1e-20]."""
    from bayesopt_smart_amd.acquisition import hypervolume_boxes
    rng = np.random.default_rng(77)
    a = np.sort(rng.uniform(0.1, 0.9, 5))
    front, r = np.stack([a, 1.0 - a], 1), np.zeros(2)
    boxes = hypervolume_boxes(front, r)
    var = rng.uniform(0.05, 2.0, (2, TAIL_N))
    mu = r[:, None] - rng.uniform(7.0, 20.0, (2, TAIL_N)) * np.sqrt(var)
    rule = X.reference(mu, var, boxes)[0]
    return front, r, boxes, mu, var, rule


def test_order_in_the_tail(bo):
    """Every value in [1e-200, 1e-20], where the earlier tolerance accepted any order: ehvi_select_indices returns
    the mpmath order of the top 16 free candidates, whose gaps exceed 10 x the bound (on the reference alone)."""
    import torch
    from bayesopt_smart_amd.acquisition import ehvi_select_indices
    from bayesopt_smart_amd.predict import CandidateSet
    front, r, boxes, mu, var, rule = _tail()
    assert rule.qualifies() and rule.held.all()
    assert all(1e-200 <= v <= 1e-20 for v in rule.ref)
    excl = np.zeros(TAIL_N, dtype=bool)
    excl[TAIL_EVALUATED] = True
    picks, gaps, nxt = LR.select_top(rule.val, excl, TAIL_Q)
    assert (gaps > 10.0 * np.maximum(rule.bound[picks], rule.bound[nxt])).all()          # on the reference alone
    assert [rule.ref[i] for i in picks] == sorted((rule.ref[i] for i in np.flatnonzero(~excl)), reverse=True)[:TAIL_Q]
    cands = CandidateSet.grid([(0, TAIL_N)])
    ev = cands.points(TAIL_EVALUATED).astype(np.float64)
    y = np.vstack([front, r[None, :] + 0.01])                # the front's points and one dominated row
    acq = torch.zeros(TAIL_N, dtype=torch.float64, device="cuda")
    idx = ehvi_select_indices(acq, torch.tensor(mu, device="cuda"), torch.tensor(var, device="cuda"), y, len(y), r, cands,
                              ev, TAIL_Q)
    miss, worst = rule.check(acq.cpu().numpy())
    print(f"tail: values {rule.val.min():.3g} .. {rule.val.max():.3g}, smallest top-16 gap / bound "
          f"{float((gaps / np.maximum(rule.bound[picks], rule.bound[nxt])).min()):.3g}; worst |E - E_ref| / bound = {worst:.3g}")
    assert miss == 0
    assert np.asarray(idx).tolist() == picks.tolist()


# the constraint bands: one-sided each way, two-sided, 1e-6 wide (test_gpu_cehvi's KINDS), in this order per case
BANDS = {1: [(k,) for k in (2, 1, 0, 3)], 2: [(2, 3), (1, 0)]}
AWAY = 40                                           # the columns AWAY .. AWAY + 19 hold means 10 sigma outside the band


@functools.lru_cache(maxsize=None)
def _con(m, kinds):
    """(bounds, mu_c, var_c, con): test_gpu_cehvi's constraint rows and special columns for the bands `kinds`,
    ten candidates 10 standard deviations under the band and ten 10 over it, and their mpmath part."""
    n = CAP[m]
    rng = np.random.default_rng(1000 * m + sum(7 ** i * k for i, k in enumerate(kinds)))
    bounds = np.array([KINDS[k] for k in kinds])
    mu_c, var_c = _constraint_rows(rng, bounds, n)
    for j, (lo, hi) in enumerate(bounds):
        sg = np.sqrt(var_c[j, AWAY:AWAY + 20])
        mu_c[j, AWAY:AWAY + 10] = (lo if np.isfinite(lo) else hi) - 10.0 * sg[:10]
        mu_c[j, AWAY + 10:AWAY + 20] = (hi if np.isfinite(hi) else lo) + 10.0 * sg[10:]
    return bounds, mu_c, var_c, X.con_part(mu_c, var_c, bounds)


@pytest.mark.parametrize("c", [1, 2])
@pytest.mark.parametrize("m", [2, 3])
def test_constrained_scan(bo, m, c):
    """acq and pof_out of the constrained scan under their rules, in the direct and the table form (same bits),
    over _case(m, "cont", 17)'s objective rows and every band."""
    import torch
    from bayesopt_smart_amd.acquisition import EhviTables
    front, r, boxes, mu_o, var_o = _case(m, "cont", 17)
    tables = EhviTables(front, r, "cuda")
    assert tables.threads > 0
    for kinds in BANDS[c]:
        bounds, mu_c, var_c, con = _con(m, kinds)
        _, p_rule, v_rule = X.combine(_box(m, "cont", 17), con, boxes.shape[0], m)
        assert v_rule.qualifies() and p_rule.low.mean() <= X.LOW_SHARE, (v_rule.fmax, v_rule.low.mean(), p_rule.low.mean())
        assert p_rule.nan.sum() >= 1 and p_rule.zero.sum() >= 1 and v_rule.nan.sum() > p_rule.nan.sum()
        mu_d = torch.tensor(np.vstack([mu_o, mu_c]), device="cuda")
        var_d = torch.tensor(np.vstack([var_o, var_c]), device="cuda")
        acq, pof = _cscan(mu_d, var_d, tables, bounds, "direct")
        (miss_v, worst_v), (miss_p, worst_p) = v_rule.check(acq), p_rule.check(pof)
        print(f"m={m} bands {bounds.tolist()}: worst |V - V_ref| / bound = {worst_v:.3g}, pof_out {worst_p:.3g}; "
              f"{int((v_rule.held & (v_rule.val < 1e-9)).sum())} of {int(v_rule.held.sum())} values below 1e-9")
        assert miss_v == 0 and miss_p == 0, (kinds, miss_v, worst_v, miss_p, worst_p)
        tacq, tpof = _cscan(mu_d, var_d, tables, bounds, "table")
        assert same_bits(tacq, acq) and same_bits(tpof, pof)


def test_kriging_believer_last_scan(bo):
    """bo_select_batch_kb, grid_case(24, 1), q = 4: acq_last is the EHVI of the means over the front extended by
    the first three believed vectors, with the variance after three picks.  Both are the device's own outputs
    (a q = 3 call's var and believed): the rule holds the scan inside the batch kernel, not its variance update."""
    from bayesopt_smart_amd.acquisition import _front_of, hypervolume_boxes
    from test_gpu_kb import GRID, cand_set, grid_case, grid_ref, ref_point_of, run
    case, ref = grid_case(24, 1), grid_ref(24, 1)
    cands = cand_set(bo, case, "grid", *GRID)
    q3 = run(bo, case, ref, cands, q=3)
    q4 = run(bo, case, ref, cands, q=4)
    assert q4["top_idx"][:3].tolist() == q3["top_idx"].tolist() and same_bits(q4["believed"][:3], q3["believed"])
    rp = ref_point_of(case)
    front = np.concatenate([_front_of(case["y"], case["y"].shape[0], rp), q3["believed"]])
    boxes = hypervolume_boxes(front, rp)
    rule = X.reference(np.asarray(ref["mu"], dtype=np.float64), np.ascontiguousarray(q3["var"], dtype=np.float64), boxes)[0]
    assert rule.qualifies(), (rule.fmax, rule.low.mean())
    miss, worst = rule.check(q4["acq_last"])
    print(f"kb: {boxes.shape[0]} boxes, {int(rule.held.sum())} candidates under the rule, "
          f"{int((rule.held & (rule.val < 1e-9)).sum())} below 1e-9: worst |E - E_ref| / bound = {worst:.3g}")
    assert miss == 0


LOOP_STRIDE = 10            # every tenth candidate of the 120 x 120 grid: 1440 mpmath values per iteration


def test_loop_acquisition_values(bo):
    """test_gpu_ehvi.test_orchestrator_ehvi_acquisition's loop: the acquisition array of each of its three
    iterations under the rule, at every tenth candidate.  A check of the data path: the reference point is -3e4
    and the values are large.  EXEMPT from the 2^10 cap on F_bk, which 3e4 exceeds: held to 2^16 instead, under
    which a subnormal psi's absolute error (2^-1074) carried through the product stays below 2^-1058, still 2^105
    under u 2^-900.  The candidates at evaluated points (the variance at its floor, the mean dominated) lie under
    2^-900 and are range-checked; their share is printed, and most candidates are under the rule."""
    from oracle import oracle_np as O
    from bayesopt_smart_amd.acquisition import hypervolume_boxes
    from bayesopt_smart_amd.bayesian_optimization import BayesianOptimization

    def toy(x):
        return np.array([-((x[0] - 60) ** 2) + 100, -((x[1] - 50) ** 2) + 20], dtype=np.float64)

    states = []
    np.random.seed(7)
    opt = BayesianOptimization(toy, [(0, 120), (0, 120)], n_objectives=2, initial_samples=6, n_iterations=3,
                               batch_size=3, acquisition="ehvi", reference_point=[-3e4, -3e4],
                               callbacks=[lambda s: states.append({k: np.array(s[k]) for k in (
                                   "iteration", "y_vector", "mu_objectives", "variance_objectives",
                                   "acquisition_values")})])
    opt.optimize()
    r = np.asarray(opt.reference_point, dtype=np.float64)
    assert len(states) == 3
    for s in states:
        it = int(s["iteration"])
        y = s["y_vector"][:it].astype(np.float64)
        front = y[O.is_pareto_efficient(y)]
        mu = np.asarray(s["mu_objectives"], dtype=np.float64)[:, ::LOOP_STRIDE]
        var = np.asarray(s["variance_objectives"], dtype=np.float64)[:, ::LOOP_STRIDE]
        rule = X.reference(mu, var, hypervolume_boxes(front, r))[0]
        assert rule.fmax <= 2.0 ** 16 and not rule.nan.any() and rule.held.mean() >= 0.5
        miss, worst = rule.check(np.asarray(s["acquisition_values"], dtype=np.float64)[::LOOP_STRIDE])
        print(f"iteration {it}: front of {front.shape[0]}, {int(rule.zero.sum())} exact zeros, {rule.low.mean():.4f} under 2^-900, values up to {rule.val.max():.3g}: "
              f"worst |E - E_ref| / bound = {worst:.3g}")
        assert miss == 0

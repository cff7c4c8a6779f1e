"""The log-space EHVI on the device (bo_log_ehvi, direct and table forms; acquisition "logehvi") against
tests/logehvi_ref.py.  PARITY UNPINNED by the reference, which has no EHVI.

The scan is held to the rounding rule of include/bo_amd.h at EVERY candidate, none left out:
    |L - L_ref| <= u [C K + n_boxes + 2],  C = 8,  and logpof_out to u [C sum_j (kappa_j + |ln P_j|) + 2];
where L_ref is -inf or NaN the device gives that value.  mu and var are built on the host and uploaded.
The selection tests assert ON THE REFERENCE ALONE that consecutive values of the selection order differ by
more than twice the bound, and then require the device's picks to equal it.  The device's worst fraction of
the bound over this file: see DESIGN.md section 19."""
import ctypes
import functools
import hashlib
import json
import os
import socket
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import ehvi_ref as ER
import logehvi_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf
N = 257
FORMS = ("direct", "table")
FRONT_POINTS = {1: 1, 2: 8, 3: 6, 4: 5}        # m = 1 has one front besides the empty one: a single point
# the seven constraints: one-sided each way, two-sided wide and thin, (-inf, +inf), and again one-sided
BOUNDS = np.array([[0.0, INF], [-INF, 1.0], [-0.5, 1.5], [0.3, 0.3 + 1e-6], [-INF, INF], [-2.0, INF], [-INF, -1.0]])


@pytest.fixture(scope="module")
def bo():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import bayesopt_smart_amd as bo
    return bo


def _front(rng, m, points):
    """`points` mutually non-dominated rows in (0, 1)^m (on a sphere's positive part)."""
    f = np.abs(rng.normal(size=(points, m))) + 0.05
    return f / np.linalg.norm(f, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def _case(m, empty):
    """(front, r, boxes, mu, var [m + 7, N]): candidates from well above the front to 1e4 standard deviations
    under it, sigma from 1e-3 to 3, and in the columns 10 .. 24 the special ones: NaN mu / var in an objective
    and in a constraint row, var = 0 above and below the front, var < 0, z = -31.9 / -32 / -40 / -1e4 / -1e6
    against the reference point, var = 0 in a constraint row inside / outside / on its bound, a constraint 45
    standard deviations outside."""
    from bayesopt_smart_amd.acquisition import hypervolume_boxes
    rng = np.random.default_rng(100 * m + int(empty))
    r = np.full(m, -0.25)
    front = np.zeros((0, m)) if empty else _front(rng, m, FRONT_POINTS[m])
    boxes = hypervolume_boxes(front, r)
    sg = 10.0 ** rng.uniform(-3.0, 0.5, (m + 7, N))
    mu = rng.uniform(-0.5, 1.2, (m + 7, N)) - sg * np.abs(rng.normal(size=(m + 7, N))) * rng.choice([0.0, 3.0, 30.0], (m + 7, N))
    mu[m:] = rng.uniform(-1.0, 1.5, (7, N)) + sg[m:] * rng.normal(size=(7, N)) * rng.choice([1.0, 10.0, 40.0], (7, N))
    var = sg * sg
    s = 10
    mu[0, s] = np.nan
    var[m - 1, s + 1] = np.nan
    mu[m, s + 2] = np.nan
    var[m + 6, s + 3] = np.nan
    mu[:m, s + 4], var[:m, s + 4] = 1.5, 0.0
    mu[:m, s + 5], var[:m, s + 5] = -0.3, 0.0
    var[:m, s + 6] = -var[:m, s + 6]
    for j, z in enumerate((-31.9, -32.0, -40.0, -1e4, -1e6)):
        mu[0, s + 7 + j], var[0, s + 7 + j] = r[0] + z * 0.5, 0.25
    mu[m, s + 12], var[m, s + 12] = 0.5, 0.0              # inside [0, inf)
    mu[m, s + 13], var[m, s + 13] = -0.5, 0.0             # outside: P = 0
    mu[m, s + 14], var[m, s + 14] = 0.0, 0.0              # on the bound: inside
    mu[m + 1, s + 15], var[m + 1, s + 15] = 1.0 + 45.0, 1.0
    for a in (front, r, boxes, mu, var):
        a.setflags(write=False)
    return front, r, boxes, mu, var


@functools.lru_cache(maxsize=None)
def _parts(m, empty):
    """The reference's box part and its seven constraint parts, computed once per case."""
    front, r, boxes, mu, var = _case(m, empty)
    return R.box_part(mu[:m], var[:m], boxes), R.con_part(mu[m:], var[m:], BOUNDS)


@functools.lru_cache(maxsize=None)
def _ref(m, empty, n_con):
    box, con = _parts(m, empty)
    return R.combine(box, con[:n_con], _case(m, empty)[2].shape[0])


def _scan(mu_d, var_d, tables, bounds, form, lp=True):
    """(L, logpof) of the device scan, numpy."""
    import torch
    from bayesopt_smart_amd.acquisition import log_expected_hypervolume_improvement
    lpo = torch.full((mu_d.shape[1],), -7.0, dtype=torch.float64, device="cuda") if lp else None
    acq = log_expected_hypervolume_improvement(mu_d, var_d, None, None, constraint_bounds=bounds, logpof_out=lpo,
                                               form=form, tables=tables)
    return acq.cpu().numpy(), (lpo.cpu().numpy() if lp else None)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64))


@pytest.mark.parametrize("empty", [True, False])
@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_rule_at_every_candidate(bo, m, empty):
    """n in {1, 63, 64, 65, 257} x both forms x n_con in {0, 1, 8 - m} (7 with one objective; BO_MAX_OBJ = 8
    outputs in all): the rule for L and for logpof_out at every candidate, the limits exactly, direct == table
    bit for bit, and a candidate's bits do not depend on n."""
    import torch
    from bayesopt_smart_amd.acquisition import EhviTables
    front, r, boxes, mu, var = _case(m, empty)
    tables = EhviTables(front, r, "cuda")
    assert tables.log_threads > 0 and tables.n_boxes == boxes.shape[0]
    worst = worst_lp = 0.0
    for n_con in (0, 1, 8 - m):
        lref, bound, lpref, lpb = _ref(m, empty, n_con)
        rows = m + n_con
        assert np.isnan(lref).sum() >= 2 and np.isneginf(lref).sum() >= 1 and np.isfinite(lref).sum() > N // 2
        whole = None
        for n in (N, 1, 63, 64, 65):
            mu_d = torch.tensor(mu[:rows, :n], device="cuda")
            var_d = torch.tensor(var[:rows, :n], device="cuda")
            got = {f: _scan(mu_d, var_d, tables, BOUNDS[:n_con], f) for f in FORMS}
            for f in FORMS:
                out, w = R.check_rule(got[f][0], lref[:n], bound[:n])
                outp, wp = R.check_rule(got[f][1], lpref[:n], lpb[:n])
                worst, worst_lp = max(worst, w), max(worst_lp, wp)
                assert out == 0.0 and outp == 0.0, (n_con, n, f, out, w, outp, wp)
            assert same_bits(got["table"][0], got["direct"][0]) and same_bits(got["table"][1], got["direct"][1])
            auto = _scan(mu_d, var_d, tables, BOUNDS[:n_con], "auto", lp=False)[0]
            assert same_bits(auto, got["direct"][0])
            if n == N:
                whole = got["direct"]
            assert same_bits(got["direct"][0], whole[0][:n]) and same_bits(got["direct"][1], whole[1][:n])
        if n_con == 0:
            assert (whole[1] == 0.0).all()
    print(f"m={m} empty={empty}: worst |L - L_ref| / bound {worst:.3g}, logpof {worst_lp:.3g}")


def test_no_boxes_and_identities(bo):
    """n_boxes = 0: -inf at every candidate (NaN where a row holds NaN), in both forms; bounds (-inf, +inf) add
    exactly 0; numpy in, numpy out with the front given as points."""
    import torch
    from bayesopt_smart_amd.acquisition import EhviTables, log_expected_hypervolume_improvement
    front, r, boxes, mu, var = _case(2, False)
    none = SimpleNamespace(n_obj=2, n_boxes=0, boxes=None, edges=None, box_idx=None, n_edges=(ctypes.c_int32 * 2)(0, 0))
    mu_d, var_d = torch.tensor(mu[:3], device="cuda"), torch.tensor(var[:3], device="cuda")
    lref = R.reference(mu[:3], var[:3], np.zeros((0, 4)), BOUNDS[:1])[0]
    assert np.isneginf(lref[~np.isnan(lref)]).all()
    for f in FORMS + ("auto",):
        got, lp = _scan(mu_d, var_d, none, BOUNDS[:1], f)
        assert same_bits(got, lref)
        assert np.isfinite(lp[~np.isnan(lp)]).sum() > 100
    tables = EhviTables(front, r, "cuda")
    plain = _scan(mu_d[:2].contiguous(), var_d[:2].contiguous(), tables, None, "direct", lp=False)[0]
    free, lp = _scan(mu_d, var_d, tables, np.array([[-INF, INF]]), "direct")
    nan_c = np.isnan(mu[2]) | np.isnan(var[2])
    assert same_bits(free[~nan_c], plain[~nan_c]) and np.isnan(free[nan_c]).all() and (lp[~nan_c] == 0.0).all()
    out = log_expected_hypervolume_improvement(mu[:2], var[:2], front, r)
    assert isinstance(out, np.ndarray) and same_bits(out, plain)
    empty = log_expected_hypervolume_improvement(mu_d[:2, :0].contiguous(), var_d[:2, :0].contiguous(), None, None, tables=tables)
    assert empty.shape == (0,)


def test_status_codes(bo):
    from bayesopt_smart_amd import _lib
    from bayesopt_smart_amd.acquisition import EhviTables, log_expected_hypervolume_improvement
    rng = np.random.default_rng(2)
    a = np.sort(rng.uniform(0.0, 1.0, 90))
    front = np.stack([a, 1.0 - a], 1)                     # 90 points: 91 + 91 edges, no 16-byte table fits
    tables = EhviTables(front, [-0.1, -0.1], "cuda")
    assert tables.sum_edges > 160 and tables.log_threads == 0 and tables.threads == 64
    mu, var = rng.normal(size=(2, 65)), np.ones((2, 65))
    with pytest.raises(_lib.BoNativeError):
        log_expected_hypervolume_improvement(mu, var, None, None, form="table", tables=tables)
    got = log_expected_hypervolume_improvement(mu, var, None, None, form="auto", tables=tables)      # the direct form
    lref, bound, _, _ = R.reference(mu, var, tables.boxes.cpu().numpy())
    assert R.check_rule(got, lref, bound)[0] == 0.0
    with pytest.raises(ValueError, match="exceeds the upper bound"):
        log_expected_hypervolume_improvement(np.zeros((3, 4)), np.ones((3, 4)), None, None, constraint_bounds=[(1.0, 0.0)],
                                             tables=tables)
    with pytest.raises(ValueError, match="mu has 3 rows"):
        log_expected_hypervolume_improvement(np.zeros((3, 4)), np.ones((3, 4)), None, None, tables=tables)


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("n_con", [0, 2])
def test_bits_shards_repeat_and_capture(bo, form, n_con):
    """Two shards through pointer offsets (ld > n) equal the single call; a second call and a captured and
    replayed call give the same bits."""
    import torch
    from bayesopt_smart_amd import _lib
    from bayesopt_smart_amd.acquisition import EhviTables
    from bayesopt_smart_amd.device import stream_handle
    front, r, boxes, mu, var = _case(3, False)
    tb = EhviTables(front, r, "cuda")
    dev = torch.device("cuda")
    rows = 3 + n_con
    mu_d, var_d = torch.tensor(mu[:rows], device=dev), torch.tensor(var[:rows], device=dev)
    lo = (ctypes.c_double * 8)(*BOUNDS[:n_con, 0])
    hi = (ctypes.c_double * 8)(*BOUNDS[:n_con, 1])
    lib = _lib.load()
    out = {k: torch.zeros(N, dtype=torch.float64, device=dev) for k in ("w", "wl", "p", "pl", "again", "al", "rep", "rl")}

    def call(acq, lp, first, count, stream):
        _lib.check(lib.bo_log_ehvi(acq.data_ptr() + 8 * first, lp.data_ptr() + 8 * first, mu_d.data_ptr() + 8 * first,
                                   var_d.data_ptr() + 8 * first, N, count, 3, n_con, lo, hi, tb.boxes.data_ptr(),
                                   tb.n_boxes, tb.edges.data_ptr(), tb.n_edges, tb.box_idx.data_ptr(), form, stream),
                   "bo_log_ehvi")

    st = stream_handle(dev)
    call(out["w"], out["wl"], 0, N, st)
    call(out["p"], out["pl"], 0, 130, st)
    call(out["p"], out["pl"], 130, N - 130, st)
    call(out["again"], out["al"], 0, N, st)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side, capture_error_mode="relaxed"):
            call(out["rep"], out["rl"], 0, N, side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert not out["rep"].any() and not out["rl"].any()          # captured, not run
    g.replay()
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in out.items()}
    lref = _ref(3, False, n_con)[0]
    assert np.array_equal(np.isnan(h["w"]), np.isnan(lref)) and np.isfinite(h["w"]).sum() > N // 2
    for a, b in (("p", "pl"), ("again", "al"), ("rep", "rl")):
        assert same_bits(h[a], h["w"]) and same_bits(h[b], h["wl"]), a


@pytest.mark.parametrize("m", [2, 3])
def test_agrees_with_the_linear_scan(bo, m):
    """Where the device's own "ehvi" value is at least 2^-500: |L - log(ehvi)| within the rule plus "ehvi"'s
    tolerance (HVI_RTOL on the box sum's scale, carried to the logarithm); and the masked top-16 of the two
    arrays is the same index list, the linear top-17 being distinct by more than that tolerance."""
    import torch
    from bayesopt_smart_amd.acquisition import (EhviTables, ehvi_select_indices, expected_hypervolume_improvement)
    from bayesopt_smart_amd.predict import CandidateSet
    front, r, boxes, mu, var = _case(m, False)
    tables = EhviTables(front, r, "cuda")
    mu_d, var_d = torch.tensor(mu[:m], device="cuda"), torch.tensor(var[:m], device="cuda")
    lin = expected_hypervolume_improvement(mu_d, var_d, None, None, tables=tables).cpu().numpy()
    got = _scan(mu_d, var_d, tables, None, "auto", lp=False)[0]
    _, bound, _, _ = _ref(m, False, 0)
    tol = ER.HVI_RTOL * ER.scale(np.nan_to_num(mu[:m]), np.nan_to_num(np.abs(var[:m])), r)
    with np.errstate(all="ignore"):
        ok = (lin >= 2.0 ** -500) & (tol < 0.5 * lin)
        tol_log = -np.log1p(-tol / lin)
        err = np.abs(got - np.log(lin))
    print(f"m={m}: {ok.sum()} candidates compared, worst |L - log ehvi| / allowance "
          f"{(err[ok] / (bound[ok] + tol_log[ok])).max():.3g}")
    assert ok.sum() > 40 and (err[ok] <= bound[ok] + tol_log[ok]).all()
    assert np.array_equal(np.isnan(got), np.isnan(lin)) and (lin[np.isneginf(got)] == 0.0).all()
    assert np.isfinite(got[lin == 0.0]).sum() > 0                # finite where the linear scan underflowed
    # the selection: a 1-D grid of N candidates, some evaluated
    cands = CandidateSet.grid([(0, N)])
    ev_idx = np.array([3, 40, 41, 200])
    ev = cands.points(ev_idx).astype(np.float64)
    keep = ~np.isnan(lin)
    mu_s, var_s = np.where(keep, mu[:m], 0.0), np.where(keep, var[:m], 1.0)       # no NaN candidate here
    mu_sd, var_sd = torch.tensor(mu_s, device="cuda"), torch.tensor(var_s, device="cuda")
    lin_s = expected_hypervolume_improvement(mu_sd, var_sd, None, None, tables=tables).cpu().numpy()
    excl = np.zeros(N, dtype=bool)
    excl[ev_idx] = True
    picks, gaps, _ = R.select_top(lin_s, excl, 16)
    assert (lin_s[picks] >= 2.0 ** -500).all() and (gaps > 1e-6 * lin_s[picks]).all()
    y = np.vstack([front, r[None, :] + 0.01])              # the front's points and one dominated row
    acq = torch.zeros(N, dtype=torch.float64, device="cuda")
    a = ehvi_select_indices(acq, mu_sd, var_sd, y, len(y), r, cands, ev, 16)
    assert same_bits(acq.cpu().numpy(), lin_s)
    b = ehvi_select_indices(acq, mu_sd, var_sd, y, len(y), r, cands, ev, 16, log=True)
    assert a.tolist() == picks.tolist() and b.tolist() == picks.tolist()


def test_minus_inf_in_the_selection(bo):
    """What bo_select_topq_masked does with -inf (include/bo_amd.h documents it): an ordinary value, the lowest.
    An array whose free candidates are ALL -inf: they are selected in index order with their own indices and
    the value -inf; the "no candidate" record differs by its index -1 alone."""
    import torch
    from bayesopt_smart_amd.acquisition import ehvi_select_indices
    from bayesopt_smart_amd.predict import CandidateSet
    n = 70
    cands = CandidateSet.grid([(0, n)])
    mu = np.full((2, n), -1.0)                             # sigma = 0 below the reference point: the exact EHVI is 0
    var = np.zeros((2, n))
    y = np.array([[0.5, 0.5]])
    ev_idx = np.array([0, 2, 5])
    ev = cands.points(ev_idx).astype(np.float64)
    acq = torch.zeros(n, dtype=torch.float64, device="cuda")
    mu_d, var_d = torch.tensor(mu, device="cuda"), torch.tensor(var, device="cuda")
    rec = ehvi_select_indices(acq, mu_d, var_d, y, 1, [0.0, 0.0], cands, ev, 5, return_record=True, log=True)
    assert np.isneginf(acq.cpu().numpy()).all()
    assert rec[5:].view(torch.int64).cpu().numpy().tolist() == [1, 3, 4, 6, 7]
    assert np.isneginf(rec[:5].cpu().numpy()).all()
    # fewer free candidates than the batch: the rest of the record is "no candidate" (-inf, -1)
    ev_all = cands.points(np.arange(2, n)).astype(np.float64)
    rec = ehvi_select_indices(acq, mu_d, var_d, y, 1, [0.0, 0.0], cands, ev_all, 5, return_record=True, log=True)
    assert rec[5:].view(torch.int64).cpu().numpy().tolist() == [0, 1, -1, -1, -1]
    assert np.isneginf(rec[:5].cpu().numpy()).all()
    # one finite value among them comes first
    mu[:, 33], var[:, 33] = 0.2, 1.0
    idx = ehvi_select_indices(acq, torch.tensor(mu, device="cuda"), torch.tensor(var, device="cuda"), y, 1, [0.0, 0.0],
                              cands, ev, 3, log=True)
    assert idx.tolist() == [33, 1, 3] and np.isfinite(acq.cpu().numpy()[33])


@functools.lru_cache(maxsize=None)
def _motivating():
    c = R.motivating_case()
    from bayesopt_smart_amd.acquisition import hypervolume_boxes
    boxes = hypervolume_boxes(c["front"], c["ref_point"])
    lref, bound, _, _ = R.reference(c["mu"], c["var"], boxes)
    return c, boxes, lref, bound


def test_motivating_case_on_the_device(bo):
    """The state of tests/test_logehvi_ref.py's motivating case (n = 1023, m = 2, the rule at every candidate,
    both forms), q = 16: "ehvi" returns a batch whose tail is the lowest free indices with value 0.0; "logehvi"
    returns the reference's top 16, in order."""
    import torch
    from bayesopt_smart_amd.acquisition import EhviTables, ehvi_select_indices
    from bayesopt_smart_amd.predict import CandidateSet
    c, boxes, lref, bound = _motivating()
    free = ~c["evaluated"]
    tables = EhviTables(c["front"], c["ref_point"], "cuda")
    mu_d, var_d = torch.tensor(c["mu"], device="cuda"), torch.tensor(c["var"], device="cuda")
    for f in ("direct",) + (("table",) if tables.log_threads else ()):
        got = _scan(mu_d, var_d, tables, None, f, lp=False)[0]
        out, worst = R.check_rule(got, lref, bound)
        print(f"{f}: n = 1023, {boxes.shape[0]} boxes: share outside the rule {out}, worst fraction of the bound {worst:.3g}")
        assert out == 0.0
    picks, gaps, nxt = R.select_top(lref, c["evaluated"], 16)
    assert (gaps > 2 * np.maximum(bound[picks], bound[nxt])).all()                       # on the reference alone
    cands = CandidateSet.grid([(R.GRID_LO[0], R.GRID_LO[0] + R.GRID_SHAPE[0]), (R.GRID_LO[1], R.GRID_LO[1] + R.GRID_SHAPE[1])])
    assert np.array_equal(cands.points(np.arange(cands.n)).astype(np.float64), c["points"])
    ev = c["points"][c["evaluated"]]
    acq = torch.zeros(cands.n, dtype=torch.float64, device="cuda")
    lin_idx = ehvi_select_indices(acq, mu_d, var_d, c["y"], len(c["y"]), c["ref_point"], cands, ev, 16)
    lin = acq.cpu().numpy()
    pos = int((lin[free] > 0.0).sum())
    assert 0 < pos < 16 and (lin[free] == 0.0).mean() >= 0.95
    assert lin_idx[:pos].tolist() == picks[:pos].tolist()
    assert lin_idx[pos:].tolist() == np.flatnonzero(free & (lin == 0.0))[:16 - pos].tolist()      # the grid's corner
    log_idx = ehvi_select_indices(acq, mu_d, var_d, c["y"], len(c["y"]), c["ref_point"], cands, ev, 16, log=True)
    assert np.isfinite(acq.cpu().numpy()).all()
    assert log_idx.tolist() == picks.tolist()
    assert log_idx[pos:].tolist() != lin_idx[pos:].tolist()


# --------------------------------------------------------------------------- the loop
BOX = [(-5, 28), (100, 131)]
# sha256 of the acquisition arrays (3 iterations, concatenated) of the "sum_ucb" and the "ehvi" loop below on the
# commit before "logehvi" existed, recorded once on an MI355X: nothing "logehvi" adds may move a bit of them
ACQ_SHA_BEFORE = {"sum_ucb": "82436506454a1975fc3ef773bfe2cbe918c50792f8bcd6695838dab264f0b77f",
                  "ehvi": "2c2ce4a3b1fe1f7042050ea31bdc0c8f5b72044b29d663621095a72f46ef99fc"}


def toy2(x):
    a, b = (x[0] + 5.0) / 33.0, (x[1] - 100.0) / 31.0
    return np.array([-(a - 0.3) ** 2 - (b - 0.6) ** 2, np.sin(3.0 * a) + 0.5 * b])


def toy2c(x):
    a, b = (x[0] + 5.0) / 33.0, (x[1] - 100.0) / 31.0
    return np.append(toy2(x), 0.6 - a - 0.5 * b)           # feasible below a line through the box


def loop(acquisition, constrained=False, states=None):
    from bayesopt_smart_amd.bayesian_optimization import BayesianOptimization
    np.random.seed(42)
    cb = None
    if states is not None:
        cb = [lambda s: states.append({k: np.array(s[k]) for k in ("iteration", "x_vector", "mu_objectives",
                                                                   "variance_objectives", "acquisition_values", "x_next")})]
    kw = dict(n_constraints=1, constraint_bounds=[(0.0, INF)]) if constrained else {}
    opt = BayesianOptimization(toy2c if constrained else toy2, BOX, n_objectives=2, initial_samples=8, n_iterations=3,
                               batch_size=3, acquisition=acquisition, reference_point=[-3.0, -3.0], callbacks=cb, **kw)
    opt.optimize()
    return opt


@pytest.mark.parametrize("constrained", [False, True])
def test_loop(bo, constrained):
    """3 iterations of batch 3 on the 33 x 31 toy: distinct unevaluated grid points; the first iteration's
    batch equals "ehvi"'s where that one's top 3 are distinct and above 2^-500."""
    log_states, lin_states = [], []
    opt = loop("logehvi", constrained, log_states)
    xs = opt.x_vector
    assert xs.shape == (17, 2) and len({tuple(r) for r in xs.tolist()}) == 17
    pts = R.grid_points()
    assert all((pts == r).all(-1).any() for r in xs[8:])
    assert len(log_states) == 3
    for s in log_states:
        acq = s["acquisition_values"]
        assert acq.shape == (pts.shape[0],) and not np.isnan(acq).any()
    loop("ehvi", constrained, lin_states)
    s0, l0 = lin_states[0], log_states[0]
    assert same_bits(s0["mu_objectives"], l0["mu_objectives"]) and same_bits(s0["variance_objectives"], l0["variance_objectives"])
    seen = (pts[:, None, :] == s0["x_vector"][None, :8, :]).all(-1).any(-1)
    lin = s0["acquisition_values"]
    picks, gaps, _ = R.select_top(lin, seen, 3)
    # the seeds are fixed: the linear top 3 are distinct and above 2^-500 here, so the comparison runs
    assert (lin[picks] >= 2.0 ** -500).all() and (gaps > 1e-9 * lin[picks]).all()
    assert l0["x_next"].tolist() == s0["x_next"].tolist() == pts[picks].tolist()
    with np.errstate(all="ignore"):
        assert np.allclose(l0["acquisition_values"][picks], np.log(lin[picks]), rtol=0, atol=1e-6)


def _acq_sha(acquisition):
    states = []
    loop(acquisition, False, states)
    return hashlib.sha256(b"".join(np.ascontiguousarray(s["acquisition_values"], dtype=np.float64).tobytes()
                                   for s in states)).hexdigest()


@pytest.mark.parametrize("acquisition", ["sum_ucb", "ehvi"])
def test_other_loops_keep_their_bits(bo, acquisition):
    sha = _acq_sha(acquisition)
    print(acquisition, sha)
    assert sha == ACQ_SHA_BEFORE[acquisition]


def test_large_batch_through_select_indices(bo):
    from bayesopt_smart_amd.bayesian_optimization import BayesianOptimization
    np.random.seed(42)
    big = BayesianOptimization(toy2, BOX, n_objectives=2, initial_samples=8, n_iterations=1, batch_size=50,
                               acquisition="logehvi", reference_point=[-3.0, -3.0])
    big.optimize()
    assert len({tuple(r) for r in big.x_vector.tolist()}) == 58


def test_loop_over_rccl_one_rank(bo):
    """One rank with BO_FORCE_COLLECTIVES=1: the records go through the all_gather; the picks equal the run
    without a process group."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env["BO_FORCE_COLLECTIVES"] = "1"
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node", "1", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join("tests", "helpers", "logehvi_rccl_loop.py"), ROOT]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    res = [json.loads(ln[7:]) for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert len(res) == 1 and res[0]["collectives"] is True
    assert res[0]["x"] == loop("logehvi").x_vector.tolist()

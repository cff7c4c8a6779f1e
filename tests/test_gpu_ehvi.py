"""Expected hypervolume improvement on the device (bo_expected_hypervolume_improvement, direct and
table forms; acquisition="ehvi") against the numpy closed form of tests/ehvi_ref.py.  PARITY
UNPINNED by the reference, which has no EHVI; tests/test_ehvi.py pins the closed form against a
Monte-Carlo mean.  Tolerance: tests/test_hvi.py's HVI_RTOL (1e-9) times prod_k psi_k(r_k) + 1, the
EHVI over an empty front (an upper bound of every term) plus one: both sides evaluate one formula
in f64.  Largest ratio |device - ref| / (prod_k psi_k(r_k) + 1) measured over
test_every_candidate_matches_the_closed_form on an MI355X: see DESIGN.md §11."""
import ctypes
import functools

import numpy as np
import pytest

import ehvi_ref as R
from oracle import oracle_np as O
from test_hvi import HVI_RTOL, _front

pytestmark = pytest.mark.gpu

FORMS = ("direct", "table", "auto")
REF = -1.0                       # the reference point's coordinates (test_hvi.py's fronts sit above it)


def _posterior(rng, m, n, front):
    """mu / var [m, n] around the front, with the special candidates in the first columns (where
    n allows): NaN mu, NaN var, var = 0, var = 1e-10 (the floor), var = 25, far below the reference
    point, far above the front, and var = 0 exactly on a front point."""
    mu = rng.normal(size=(m, n)) * 2.0 + 1.5
    var = rng.uniform(0.01, 4.0, size=(m, n))
    if n > 9:
        mu[0, 1] = np.nan
        var[m - 1, 2] = np.nan
        var[:, 3] = 0.0
        var[:, 4] = 1e-10
        var[:, 5] = 25.0
        mu[:, 6] = -50.0
        mu[:, 7] = 60.0
        ok = front[~np.isnan(front).any(axis=1)]
        mu[:, 8] = ok[0] if ok.shape[0] else 0.0
        var[:, 8] = 0.0
        var[0, 9] = -0.3                                     # sigma = sqrt(|var|), the UCB's convention
    return mu, var


def _close(got, ref, mu, var, r):
    """(all within tolerance, largest |got - ref| / scale); NaN must meet NaN."""
    nan = np.isnan(ref)
    if not np.array_equal(np.isnan(got), nan):
        return False, np.inf
    ratio = np.abs(got[~nan] - ref[~nan]) / R.scale(mu[:, ~nan], var[:, ~nan], r)
    worst = float(ratio.max()) if ratio.size else 0.0
    return worst <= HVI_RTOL, worst


@functools.lru_cache(maxsize=None)
def _case(m, kind, p):
    from bayesopt_smart_amd.acquisition import hypervolume_boxes
    rng = np.random.default_rng(31 * m + p + (kind == "int"))
    front = _front(rng, p, m, kind)
    r = np.full(m, REF)
    mu, var = _posterior(rng, m, 3000, front)
    ref = R.ehvi(mu, var, hypervolume_boxes(front, r))
    for a in (mu, var, ref):
        a.setflags(write=False)
    return front, r, mu, var, ref


@pytest.mark.parametrize("p", [12, 17])
@pytest.mark.parametrize("kind", ["int", "cont"])
@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_every_candidate_matches_the_closed_form(m, kind, p):
    """n in {1, 255, 257, 3000} x the three forms; the table form equals the direct form bit for
    bit (one psi, one box order, the fma written out); EHVI >= 0."""
    import torch
    from bayesopt_smart_amd.acquisition import EhviTables, expected_hypervolume_improvement
    front, r, mu, var, ref = _case(m, kind, p)
    tables = EhviTables(front, r, "cuda")
    assert tables.threads == R.table_threads(tables.sum_edges) and tables.threads > 0
    worst = 0.0
    for n in (1, 255, 257, 3000):
        mu_d = torch.tensor(mu[:, :n], device="cuda")           # copies: the case is shared
        var_d = torch.tensor(var[:, :n], device="cuda")
        got = {f: expected_hypervolume_improvement(mu_d, var_d, None, None, form=f, tables=tables).cpu().numpy()
               for f in FORMS}
        for f in FORMS:
            ok, w = _close(got[f], ref[:n], mu[:, :n], var[:, :n], r)
            worst = max(worst, w)
            assert ok, (f, n, w)
            assert np.all(got[f][~np.isnan(got[f])] >= 0.0)
        assert np.array_equal(got["table"], got["direct"], equal_nan=True)
        assert np.array_equal(got["auto"], got["direct"], equal_nan=True)
    print(f"m={m} {kind} p={p}: largest |device - ref| / (prod psi(r) + 1) = {worst:.3e}")
    # numpy in, numpy out, the front given as points
    out = expected_hypervolume_improvement(mu[:, :257], var[:, :257], front, r)
    assert isinstance(out, np.ndarray) and np.array_equal(out, got["direct"][:257], equal_nan=True)


def _staircase(p):
    """p mutually non-dominated points with distinct coordinates: p + 1 boxes, and (in 2-D, where
    each box has its own column and its own floor) sum_k E_k = 2 (p + 1)."""
    t = (np.arange(p) + 0.5) / p
    return np.stack([4.0 * t, 4.0 * (1.0 - t) ** 1.5 + 0.01 * np.arange(p)[::-1] / p], axis=1)


def test_admission_thresholds():
    """m = 2 fronts whose sum_k E_k sits at and around each workgroup-size threshold of the table
    form (in 2-D the sum is even: 2 per box), and one too large for any table.  The sizes come from
    the rule's mirror; auto is right on all of them, form 2 is refused exactly where the mirror
    says so."""
    import torch
    from bayesopt_smart_amd import _lib
    from bayesopt_smart_amd.acquisition import EhviTables, expected_hypervolume_improvement
    limits = [max(s for s in range(2, 1000, 2) if R.table_threads(s) == t) for t in R.TABLE_THREADS]
    assert limits == [80, 160, 320]
    sums = sorted({s + d for s in limits for d in (-2, 0, 2)} | {400})
    rng = np.random.default_rng(9)
    r = np.full(2, REF)
    n = 300
    seen = set()
    for s in sums:
        front = _staircase(s // 2 - 1)
        tables = EhviTables(front, r, "cuda")
        assert tables.sum_edges == s and tables.n_boxes == s // 2
        want_t = R.table_threads(s)
        assert tables.threads == want_t
        seen.add(want_t)
        mu, var = _posterior(rng, 2, n, front)
        ref = R.ehvi(mu, var, tables.boxes.cpu().numpy())
        mu_d, var_d = torch.as_tensor(mu, device="cuda"), torch.as_tensor(var, device="cuda")
        auto = expected_hypervolume_improvement(mu_d, var_d, None, None, tables=tables).cpu().numpy()
        ok, w = _close(auto, ref, mu, var, r)
        assert ok, (s, w)
        if want_t:
            tab = expected_hypervolume_improvement(mu_d, var_d, None, None, form="table", tables=tables)
            assert np.array_equal(tab.cpu().numpy(), auto, equal_nan=True)
        else:
            with pytest.raises(_lib.BoNativeError) as e:
                expected_hypervolume_improvement(mu_d, var_d, None, None, form="table", tables=tables)
            assert e.value.status == _lib.ERR_UNSUPPORTED
    assert seen == {256, 128, 64, 0}


@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_empty_front(m):
    """EHVI over an empty front = prod_k psi_k(r_k), rel 1e-12.  The posteriors keep
    z = (mu - r) / sigma >= -4: the closed form of ehvi_ref (phi + z Phi, the textbook statement)
    cancels for z < 0 and is itself good to about z^4 2^-52 only -- exp(-z^2/2) and
    erfc(|z| / sqrt 2) each carry z^2 2^-52 from their rounded arguments and the difference keeps
    1 / z^2 of them -- which is 6e-14 at z = -4 and passes 1e-12 near z = -8.  The tail is
    test_psi_tail's."""
    import torch
    from bayesopt_smart_amd.acquisition import expected_hypervolume_improvement
    rng = np.random.default_rng(m)
    mu = rng.uniform(-3.0, 4.0, size=(m, 1000))
    var = rng.uniform(0.25, 4.0, size=(m, 1000))
    r = np.full(m, REF)
    want = np.prod([R.psi(mu[k], np.sqrt(var[k]), r[k]) for k in range(m)], axis=0)     # prod_k psi_k(r_k)
    for f in FORMS:
        got = expected_hypervolume_improvement(torch.as_tensor(mu, device="cuda"), torch.as_tensor(var, device="cuda"),
                                               np.zeros((0, m)), r, form=f).cpu().numpy()
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
        assert np.all(got >= 0)


def test_psi_tail():
    """psi far below the bound, z = -t in [-30, -4], where the textbook form has lost its digits
    (test_empty_front): the device's psi against sigma exp(-t^2/2) (1/sqrt(2 pi) - t erfcx(t/sqrt 2)/2)
    in numpy with scipy's erfcx -- the device's own rearrangement, so this checks its exp and erfcx,
    not the formula.  sigma is a power of two, so both sides hold the same t; what is left is the
    two libraries' last bits of erfcx, of which the difference keeps t^2 <= 900 times (about 4e-13
    for two ulps), and of exp: rel 1e-12.  psi is positive and decreasing all the way."""
    import torch
    from scipy.special import erfcx
    from bayesopt_smart_amd.acquisition import expected_hypervolume_improvement
    t = np.linspace(4.0, 30.0, 1000)
    worst = 0.0
    for sigma in (0.5, 1.0, 2.0):
        mu = (REF - sigma * t)[None, :]
        var = np.full_like(mu, sigma * sigma)
        tt = -(mu[0] - REF) / sigma
        want = sigma * np.exp(-0.5 * (tt * tt)) * (0.3989422804014327 - (0.5 * tt) * erfcx(tt * 0.7071067811865476))
        for f in ("direct", "table"):
            got = expected_hypervolume_improvement(torch.as_tensor(mu, device="cuda"), torch.as_tensor(var, device="cuda"),
                                                   np.zeros((0, 1)), np.array([REF]), form=f).cpu().numpy()
            rel = np.abs(got - want) / want
            worst = max(worst, float(rel.max()))
            assert np.all(rel <= 1e-12), rel.max()
            assert np.all(got > 0) and np.all(np.diff(got) < 0)
    print(f"psi tail: largest relative difference {worst:.3e}")


@pytest.mark.parametrize("form", [1, 2])
def test_shards_through_pointer_offsets(form):
    """Two calls over [0, 1500) and [1500, 3000) of one [m][3000] array equal the single call."""
    import torch
    from bayesopt_smart_amd import _lib
    from bayesopt_smart_amd.acquisition import EhviTables
    from bayesopt_smart_amd.device import stream_handle
    front, r, mu, var, _ = _case(3, "cont", 17)
    tb = EhviTables(front, r, "cuda")
    dev = torch.device("cuda")
    mu_d, var_d = torch.tensor(mu, device=dev), torch.tensor(var, device=dev)      # copies: the case is shared
    whole = torch.zeros(3000, dtype=torch.float64, device=dev)
    parts = torch.zeros(3000, dtype=torch.float64, device=dev)
    lib = _lib.load()

    def call(out, first, count):
        _lib.check(lib.bo_expected_hypervolume_improvement(
            out.data_ptr() + 8 * first, mu_d.data_ptr() + 8 * first, var_d.data_ptr() + 8 * first, 3000, count, 3,
            tb.boxes.data_ptr(), tb.n_boxes, tb.edges.data_ptr(), tb.n_edges, tb.box_idx.data_ptr(), form,
            stream_handle(dev)), "bo_expected_hypervolume_improvement")

    call(whole, 0, 3000)
    call(parts, 0, 1500)
    call(parts, 1500, 1500)
    assert np.array_equal(whole.cpu().numpy(), parts.cpu().numpy(), equal_nan=True)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("kind,m,q", [("grid", 2, 3), ("sobol", 3, 5)])
def test_ehvi_select_indices(kind, m, q, masked):
    """The scan and the masked top-q: the acq array is the closed form of the mu / var given, the
    indices are select_next_batch's (the oracle's deterministic order) over the device's array
    with the evaluated points excluded -- one of them the best candidate of all."""
    import torch
    from bayesopt_smart_amd.acquisition import (ExclusionMask, ehvi_select_indices,
                                                expected_hypervolume_improvement, hypervolume_boxes)
    from bayesopt_smart_amd.predict import CandidateSet
    rng = np.random.default_rng(17 * m + q)
    cands = CandidateSet.grid([(0, 64), (0, 96)]) if kind == "grid" else CandidateSet.sobol_set(3, 20_000, scale=50.0)
    n = cands.n
    y = rng.normal(size=(40, m))
    front = y[O.is_pareto_efficient(y)]
    r = np.full(m, -4.0)
    mu = rng.normal(size=(m, n))
    var = rng.uniform(0.01, 2.0, size=(m, n))
    mu[:, 17] = np.nan                                      # a NaN candidate is selected first
    mu_d, var_d = torch.as_tensor(mu, device="cuda"), torch.as_tensor(var, device="cuda")
    scan = expected_hypervolume_improvement(mu_d, var_d, front, r).cpu().numpy()
    ok, w = _close(scan, R.ehvi(mu, var, hypervolume_boxes(front, r)), mu, var, r)
    assert ok, w
    top = int(np.nanargmax(scan))                           # an evaluated point at the top of the order
    ev_idx = np.r_[top, rng.choice(np.setdiff1d(np.arange(n), [top, 17]), 39, replace=False)]
    ev = cands.points(ev_idx).astype(np.float64)
    acq = torch.zeros(n, dtype=torch.float64, device="cuda")
    mask = ExclusionMask(cands, 0, n, "cuda").update(ev[:25]) if masked else None
    idx = ehvi_select_indices(acq, mu_d, var_d, y, 40, r, cands, ev, q, mask=mask)
    assert np.array_equal(acq.cpu().numpy(), scan, equal_nan=True)
    excl = np.zeros(n, dtype=bool)
    excl[ev_idx] = True
    want = O.select_next_batch_indices(scan, excl, q)
    assert want[0] == 17 and top not in want
    np.testing.assert_array_equal(idx, want)
    rec = ehvi_select_indices(acq, mu_d, var_d, y, 40, r, cands, ev, q, mask=mask, return_record=True)
    assert rec.shape == (2 * q,)
    np.testing.assert_array_equal(rec[q:].view(torch.int64).cpu().numpy(), want)
    np.testing.assert_array_equal(rec[:q].cpu().numpy()[1:], scan[want][1:])


def test_orchestrator_ehvi_acquisition():
    """acquisition="ehvi" through the loop: in every iteration the acquisition array is the closed
    form of that iteration's mu_objectives / variance_objectives over the Pareto front of the
    points evaluated before it, and x_next is the oracle's selection over the device's array."""
    from bayesopt_smart_amd.acquisition import hypervolume_boxes
    from bayesopt_smart_amd.bayesian_optimization import BayesianOptimization

    def toy(x):
        return np.array([-((x[0] - 60) ** 2) + 100, -((x[1] - 50) ** 2) + 20], dtype=np.float64)

    states = []
    np.random.seed(7)
    opt = BayesianOptimization(toy, [(0, 120), (0, 120)], n_objectives=2, initial_samples=6, n_iterations=3,
                               batch_size=3, acquisition="ehvi", reference_point=[-3e4, -3e4],
                               callbacks=[lambda s: states.append({k: np.array(s[k]) for k in (
                                   "iteration", "x_vector", "y_vector", "mu_objectives", "variance_objectives",
                                   "acquisition_values", "x_next")})])
    opt.optimize()
    grid = O.grid_points([(0, 120), (0, 120)])
    r = np.asarray(opt.reference_point, dtype=np.float64)
    assert len(states) == 3
    for s in states:
        it = int(s["iteration"])
        y = s["y_vector"][:it].astype(np.float64)
        front = y[O.is_pareto_efficient(y)]
        mu, var, acq = s["mu_objectives"], s["variance_objectives"], s["acquisition_values"]
        ok, w = _close(acq, R.ehvi(mu, var, hypervolume_boxes(front, r)), mu, var, r)
        assert ok, (it, w)
        np.testing.assert_array_equal(s["x_next"], O.select_next_batch(grid, acq, s["x_vector"][:it], 3))


def test_graph_capture_replays_the_scan():
    import torch
    from bayesopt_smart_amd import _lib
    from bayesopt_smart_amd.acquisition import EhviTables
    front, r, mu, var, _ = _case(2, "cont", 17)
    tb = EhviTables(front, r, "cuda")
    dev = torch.device("cuda")
    mu_d, var_d = torch.tensor(mu, device=dev), torch.tensor(var, device=dev)      # copies: the case is shared
    lib = _lib.load()
    for form in (1, 2):
        plain = torch.zeros(3000, dtype=torch.float64, device=dev)
        replay = torch.zeros(3000, dtype=torch.float64, device=dev)

        def call(out, stream):
            _lib.check(lib.bo_expected_hypervolume_improvement(
                out.data_ptr(), mu_d.data_ptr(), var_d.data_ptr(), 3000, 3000, 2, tb.boxes.data_ptr(), tb.n_boxes,
                tb.edges.data_ptr(), tb.n_edges, tb.box_idx.data_ptr(), form, stream),
                "bo_expected_hypervolume_improvement")

        call(plain, torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side, capture_error_mode="relaxed"):
                call(replay, side.cuda_stream)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        assert not replay.any()                               # captured, not run
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(replay.cpu().numpy(), plain.cpu().numpy(), equal_nan=True)

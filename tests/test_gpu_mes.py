"""Max-value entropy search (acquisition "mes": bo_path_maxima, bo_max_value_entropy,
acquisition.path_maxima / max_value_entropy / mes_select_indices) against tests/mes_ref.py.

The maxima are exact: they are compared bit for bit with fma(scale, nanmax, shift) rounded once.  The scan
is held to the rounding rule of include/bo_amd.h at EVERY candidate, with the device's own y* as data:
    |acq - acq_ref| <= u/S sum_sk [32 (1 + gamma_sk^2 / 2) + S n_obj] g_ref(gamma_sk) + 2^-1022.
A different pick changes nothing later here (one array, one top-q), but the order of near-equal values is
not defined below the bound, so the selection tests assert ON THE REFERENCE ALONE that consecutive values of
the selection order differ by more than 10 bounds, and then require the device's picks to equal it."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import mes_ref as R
from test_gpu_ts import cand_set, grid_case, grid_points

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bo():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import bayesopt_smart_amd as bo
    return bo


# --------------------------------------------------------------------------- maxima
def maxima_case(n_cand, n_s, n_obj, rot):
    """paths [S n_obj, ld = n_cand + 5] with the pad +inf (a read past n_cand shows), row r of pattern
    (r + rot) mod 8: plain; maximum at column 0; at the last column; duplicated; with -inf entries; with a
    few NaN (one of them where the maximum was); all NaN; all -inf."""
    rng = np.random.default_rng(1000 * n_cand + 10 * n_s + n_obj + rot)
    rows, ld = n_s * n_obj, n_cand + 5
    p = np.full((rows, ld), np.inf)
    p[:, :n_cand] = rng.standard_normal((rows, n_cand))
    for r in range(rows):
        row, pat = p[r, :n_cand], (r + rot) % 8
        if pat == 1:
            row[0] = 7.5
        elif pat == 2:
            row[-1] = 7.25
        elif pat == 3:
            row[rng.integers(0, n_cand, 3)] = 6.125
        elif pat == 4:
            row[rng.integers(0, n_cand, max(1, n_cand // 3))] = -np.inf
        elif pat == 5:
            row[np.argmax(row)] = np.nan
            row[rng.integers(0, n_cand, 3)] = np.nan
        elif pat == 6:
            row[:] = np.nan
        elif pat == 7:
            row[:] = -np.inf
    pm = rng.uniform(-2.0, 2.0, n_obj)
    pv = rng.uniform(0.3, 3.0, n_obj)
    return p, pm, pv


def device_maxima(p, n_cand, n_s, n_obj, pm, pv, lo=0, hi=None):
    import torch
    from bayesopt_smart_amd.acquisition import path_maxima
    hi = n_cand if hi is None else hi
    t = torch.as_tensor(p, device="cuda").reshape(n_s, n_obj, p.shape[1])
    return path_maxima(t[:, :, lo:hi], pm, pv).cpu().numpy()


def same_bits(a, b):
    """Equal bit for bit, any NaN standing for any NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64))


@pytest.mark.parametrize("n_s,n_obj", [(1, 1), (3, 2), (48, 8)])
@pytest.mark.parametrize("n_cand", [1, 63, 64, 65, 1000, 33 * 31])
def test_maxima_bits(bo, n_cand, n_s, n_obj):
    for rot in (range(8) if n_s * n_obj == 1 else (0, 3)):
        p, pm, pv = maxima_case(n_cand, n_s, n_obj, rot)
        got = device_maxima(p, n_cand, n_s, n_obj, pm, pv)
        want = R.maxima_ref(p[:, :n_cand], pm, np.sqrt(pv)).reshape(n_s, n_obj)
        assert got.shape == (n_s, n_obj)
        assert same_bits(got, want), (n_cand, n_s, n_obj, rot, got, want)
        flat = got.ravel()
        for r in range(flat.size):                 # the all-NaN and the all--inf rows
            assert not (r + rot) % 8 == 6 or np.isnan(flat[r])
            assert not (r + rot) % 8 == 7 or flat[r] == -np.inf


def test_maxima_more_than_one_chunk(bo):
    """20 000 columns: three partial maxima per row (8192 columns each), the maximum in each in turn."""
    for where in (5, 9000, 19999):
        p, pm, pv = maxima_case(20000, 3, 2, 0)
        p[:, where] = 9.0 + np.arange(6)
        p[4, where] = np.nan                       # pattern 4 has -inf entries; its maximum stays finite
        got = device_maxima(p, 20000, 3, 2, pm, pv)
        want = R.maxima_ref(p[:, :20000], pm, np.sqrt(pv)).reshape(3, 2)
        assert np.array_equal(got, want)


def test_maxima_two_shards_give_the_unsharded_bits(bo):
    p, pm, pv = maxima_case(1023, 3, 2, 0)
    p[0, 400:1023] = np.nan                        # a shard whose row is all NaN is ignored by the host max
    whole = device_maxima(p, 1023, 3, 2, pm, pv)
    a = device_maxima(p, 1023, 3, 2, pm, pv, 0, 400)
    b = device_maxima(p, 1023, 3, 2, pm, pv, 400, 1023)
    assert np.isnan(b[0, 0]) and not np.isnan(a[0, 0])
    both = np.fmax(a, b)
    assert np.array_equal(both.view(np.int64), whole.view(np.int64))


def test_maxima_empty_shard_is_nan(bo):
    p, pm, pv = maxima_case(4, 3, 2, 0)
    assert np.isnan(device_maxima(p, 4, 3, 2, pm, pv, 2, 2)).all()


# --------------------------------------------------------------------------- scan
def gammas(n, rng):
    """n target values of gamma covering [-1e6, 38], 0, +-tiny, both sides of -2^27 and +-inf (as many of
    them as n allows, the specials first)."""
    c = R.CUT
    special = [0.0, 1e-300, -1e-300, 5e-324, -5e-324, c, np.nextafter(c, 0.0), np.nextafter(c, -np.inf),
               c * (1 + 1e-9), c * (1 - 1e-9), np.inf, -np.inf, -1e6, 38.0, -0.003, 1e-8, -1e-8]
    rest = max(n - len(special), 0)
    neg = -np.exp(rng.uniform(np.log(1e-6), np.log(1e6), rest // 2))
    lin = rng.uniform(-12.0, 38.0, rest - rest // 2)
    return np.concatenate([special, neg, lin])[:n] if n >= 3 else np.array([-0.7, 0.0, 3.0])[:n]


def scan_case(n, n_obj, n_s, seed):
    """mu, var [n_obj, n] and ystar [S, n_obj]: draw 0's maxima are 0, so that gamma_0k(i) = -mu / sigma is
    the target exactly where sigma = 1 (the specials); the other draws shift it by ystar_sk / sigma."""
    rng = np.random.default_rng(seed)
    t = gammas(n, rng)
    mu, var = np.empty((n_obj, n)), np.empty((n_obj, n))
    for k in range(n_obj):
        tk = np.roll(t, 5 * k)
        sg = np.where((np.arange(n) < 17) | (np.arange(n) % 2 == 0), 1.0, rng.uniform(0.05, 4.0, n))
        sg = np.roll(sg, 5 * k)
        var[k] = sg * sg * np.where(rng.uniform(size=n) < 0.1, -1.0, 1.0)      # |var|: the sign is ignored
        with np.errstate(invalid="ignore"):
            mu[k] = -(tk * sg)
    ystar = np.zeros((n_s, n_obj))
    ystar[1:] = rng.uniform(-1.5, 2.5, (n_s - 1, n_obj))
    return mu, var, ystar


def device_scan(mu, var, ystar):
    from bayesopt_smart_amd.acquisition import max_value_entropy
    return max_value_entropy(np.ascontiguousarray(mu), np.ascontiguousarray(var), np.ascontiguousarray(ystar))


@pytest.mark.parametrize("n,n_obj,n_s", [(1, 1, 1), (1, 8, 48), (65, 2, 48), (65, 8, 3), (65, 5, 1), (1023, 1, 1),
                                         (1023, 2, 3), (1023, 5, 3)])
def test_scan_meets_the_rounding_rule(bo, n, n_obj, n_s):
    mu, var, ystar = scan_case(n, n_obj, n_s, 17 * n + n_obj + n_s)
    got = device_scan(mu, var, ystar)
    ref, bound = R.acquisition_ref(mu, var, ystar)
    out, worst = R.check_rule(got, ref, bound)
    print(f"n {n} n_obj {n_obj} S {n_s}: share outside the rule {out}, worst |err| / bound {worst:.3g} "
          f"(of 32 units: {32 * worst:.3g}), non-finite references {int((~np.isfinite(ref)).sum())}")
    assert out == 0.0, (n, n_obj, n_s, out, worst)
    fin = np.isfinite(ref)
    assert (got[fin] >= 0).all()
    if n >= 65:                                    # the covered range, on the draw whose maxima are 0
        g0 = -mu[0] / np.sqrt(np.abs(var[0]))
        assert np.nanmin(g0) == -np.inf and np.nanmax(g0) == np.inf
        assert (g0 == 0).any() and (g0 <= -1e6).any() and (g0 >= 37.9).any()
        assert (g0 == np.nextafter(R.CUT, 0.0)).any() and (g0 == np.nextafter(R.CUT, -np.inf)).any()


def test_scan_shard_independence_and_determinism(bo):
    mu, var, ystar = scan_case(1023, 5, 3, 99)
    whole = device_scan(mu, var, ystar)
    again = device_scan(mu, var, ystar)
    part = device_scan(mu[:, 300:813], var[:, 300:813], ystar)
    one = device_scan(mu[:, 700:701], var[:, 700:701], ystar)
    assert np.array_equal(whole.view(np.int64), again.view(np.int64))
    assert np.array_equal(part.view(np.int64), whole[300:813].view(np.int64))
    assert np.array_equal(one.view(np.int64), whole[700:701].view(np.int64))


def test_scan_limits(bo):
    nan, inf = np.nan, np.inf
    # one objective, one draw, y* = 0.5: sigma = 0 on both sides of and at mu = y*; NaN in mu, in var
    mu = np.array([[0.0, 0.5, 1.0, nan, 0.0, 0.0, -inf, inf]])
    var = np.array([[0.0, 0.0, 0.0, 1.0, nan, -4.0, 1.0, 1.0]])
    got = device_scan(mu, var, np.array([[0.5]]))
    assert got[0] == 0.0 and got[1] == 0.0 and got[2] == inf and np.isnan(got[3]) and np.isnan(got[4])
    assert abs(got[5] - float(R.g_mp(0.25))) <= 64 * R.U           # sigma = sqrt(|var|)
    assert got[6] == 0.0 and got[7] == inf                         # gamma = +inf / -inf through mu
    # y* = +inf gives 0, -inf gives +inf, NaN gives NaN -- with sigma > 0 and with sigma = 0
    mu2, var2 = np.array([[0.3, 0.3]]), np.array([[2.0, 0.0]])
    assert (device_scan(mu2, var2, np.array([[inf]])) == 0.0).all()
    assert (device_scan(mu2, var2, np.array([[-inf]])) == inf).all()
    assert np.isnan(device_scan(mu2, var2, np.array([[nan]]))).all()
    # NaN wins over +inf whatever the order of the terms; one NaN among S n_obj terms is enough
    mu3 = np.array([[0.0, 0.0], [nan, 0.0], [0.0, 0.0]])
    var3 = np.array([[0.0, 1.0], [1.0, 1.0], [1.0, 1.0]])
    ys3 = np.array([[-1.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    got = device_scan(mu3, var3, ys3)
    assert np.isnan(got[0]) and np.isfinite(got[1])
    ys3[1, 2] = nan
    assert np.isnan(device_scan(mu3, var3, ys3)).all()
    # g(0) = ln 2, the mean over S and the sum over the objectives
    got = device_scan(np.zeros((2, 1)), np.ones((2, 1)), np.zeros((4, 2)))
    assert abs(got[0] - 2 * np.log(2.0)) <= 16 * R.U


# --------------------------------------------------------------------------- the chain
def chain(bo, case, n_s, q=5):
    """predict -> sample_paths -> path_maxima -> max_value_entropy -> masked top-q on the 33 x 31 grid."""
    import torch
    from bayesopt_smart_amd import acquisition as A
    cands = cand_set(bo, case, "grid", (-5, 100), (33, 31))
    n_obj = len(case["pv"])
    out = bo.predict.predict_acquire(case["x"], case["y"], case["kinv"], cands, case["pm"], case["pv"], case["ls"],
                                     np.full(n_obj, 2.0), outputs=("mu", "var"))
    mu, var = out["mu"].contiguous(), out["var"].contiguous()
    paths = A.sample_paths(case["x"], case["y"], case["kinv"], cands, case["pm"], case["pv"], case["ls"],
                           case["draws"], jitter=case["lam"], device="cuda")
    ystar = A.path_maxima(paths, case["pm"], case["pv"])
    acq = A.max_value_entropy(mu, var, ystar)
    # the same through the one call the loop makes
    acq2 = torch.empty_like(acq)
    idx = A.mes_select_indices(acq2, mu, var, case["x"], case["y"], case["kinv"], cands, case["pm"], case["pv"],
                               case["ls"], case["draws"], case["x"], q, jitter=case["lam"])
    assert torch.equal(acq, acq2)
    return dict(mu=mu.cpu().numpy(), var=var.cpu().numpy(), paths=paths.cpu().numpy(), ystar=ystar.cpu().numpy(),
                acq=acq.cpu().numpy(), idx=np.asarray(idx))


@pytest.mark.parametrize("n_obj", [2, 5])
def test_chain_picks_equal_the_reference(bo, n_obj):
    case = grid_case(64, 4, n=24, n_obj=n_obj, ls=(4.0, 6.0, 5.0, 7.0, 4.5)[:n_obj] if n_obj > 2 else (4.0, 6.0))
    d = chain(bo, case, 4)
    # the maxima are those of the paths, evaluated points included
    want = R.maxima_ref(d["paths"].reshape(4 * n_obj, -1), case["pm"], np.sqrt(case["pv"])).reshape(4, n_obj)
    assert np.array_equal(d["ystar"], want)
    ref, bound = R.acquisition_ref(d["mu"], d["var"], d["ystar"])
    out, worst = R.check_rule(d["acq"], ref, bound)
    print(f"chain n_obj {n_obj}: share outside the rule {out}, worst |err| / bound {worst:.3g}")
    assert out == 0.0
    excluded = (case["pts"][:, None, :] == case["x"][None, :, :]).all(-1).any(-1)
    assert excluded.sum() == 24
    picks, gaps, nxt = R.select_top(ref, excluded, 5)
    tol = np.maximum(bound[picks], bound[nxt])
    print("picks", picks.tolist(), "gaps", gaps.tolist(), "bounds", tol.tolist())
    assert (gaps > 10 * tol).all(), (gaps, tol)                    # on the reference alone
    assert d["idx"].tolist() == picks.tolist()
    assert not excluded[d["idx"]].any()                            # evaluated points are never picked


# --------------------------------------------------------------------------- the loop
def toy5(x):
    a, b = (x[0] + 5.0) / 33.0, (x[1] - 100.0) / 31.0
    return np.array([-(a - 0.3) ** 2 - (b - 0.6) ** 2, np.sin(3.0 * a) + 0.5 * b, -(a - 0.8) ** 2 + 0.3 * np.cos(4.0 * b),
                     0.7 * a - (b - 0.2) ** 2, np.cos(2.0 * a + b)])


BOUNDS = [(-5, 28), (100, 131)]
# the picks of acquisition="sum_ucb" on toy5 (np.random.seed(42), 8 initial samples, 3 iterations of 3) on the
# commit before "mes" existed, recorded once: nothing "mes" adds may move them
SUM_UCB_PICKS = [[-5.0, 130.0], [-4.0, 130.0], [-5.0, 129.0], [27.0, 100.0], [26.0, 100.0], [27.0, 101.0],
                 [11.0, 100.0], [10.0, 100.0], [12.0, 100.0]]


def loop(acquisition, ts_seed=7, callbacks=None, record=None, **kw):
    from bayesopt_smart_amd import acquisition as A
    from bayesopt_smart_amd import bayesian_optimization as B
    np.random.seed(42)
    opt = B.BayesianOptimization(toy5, BOUNDS, n_objectives=5, initial_samples=8, n_iterations=3, batch_size=3,
                                 acquisition=acquisition, mes_samples=4, ts_features=128, ts_seed=ts_seed,
                                 callbacks=callbacks, **kw)
    inner = A.path_maxima
    if record is not None:
        def spy(*a, **k):
            y = inner(*a, **k)
            record.append(y.cpu().numpy().copy())
            return y
        A.path_maxima = spy
    try:
        opt.optimize()
    finally:
        A.path_maxima = inner
    return opt


def test_ehvi_refuses_what_mes_runs(bo):
    from bayesopt_smart_amd import bayesian_optimization as B
    with pytest.raises(ValueError, match="at most 4 objectives"):
        B.BayesianOptimization(toy5, BOUNDS, n_objectives=5, initial_samples=8, n_iterations=3, batch_size=3,
                               acquisition="ehvi")


def test_loop(bo):
    states, ystars = [], []

    def cb(state):
        states.append({k: np.array(state[k]) for k in ("mu_objectives", "variance_objectives", "acquisition_values",
                                                       "x_next")})
    opt = loop("mes", callbacks=[cb], record=ystars)
    xs = opt.x_vector
    assert xs.shape == (17, 2) and len({tuple(r) for r in xs.tolist()}) == 17      # 9 new, all distinct
    pts = grid_points((-5, 100), (33, 31))
    assert all((pts == r).all(-1).any() for r in xs[8:])                            # grid points
    assert len(states) == 3 and len(ystars) == 3 and ystars[0].shape == (4, 5)
    for it in (2,):                                                                 # the rule, from that iteration's state
        s = states[it]
        ref, bound = R.acquisition_ref(s["mu_objectives"], s["variance_objectives"], ystars[it])
        out, worst = R.check_rule(s["acquisition_values"], ref, bound)
        print(f"loop iteration {it}: share outside the rule {out}, worst |err| / bound {worst:.3g}")
        assert out == 0.0
        # and the batch is the reference's top 3 among the points not evaluated before it
        seen = (pts[:, None, :] == xs[None, : 8 + 3 * it, :]).all(-1).any(-1)
        picks, gaps, nxt = R.select_top(ref, seen, 3)
        if (gaps > 10 * np.maximum(bound[picks], bound[nxt])).all():
            assert pts[picks].tolist() == s["x_next"].tolist()
    again = loop("mes")
    other = loop("mes", ts_seed=8)
    assert np.array_equal(again.x_vector, xs)
    assert not np.array_equal(other.x_vector, xs)


def test_loop_sum_ucb_is_unchanged(bo):
    opt = loop("sum_ucb")
    print("sum_ucb picks", opt.x_vector[8:].tolist())
    assert opt.x_vector[8:].tolist() == SUM_UCB_PICKS


def test_loop_float32_branch_and_large_batch(bo):
    from bayesopt_smart_amd import bayesian_optimization as B
    opt = loop("mes", float_type=np.float32)
    assert len({tuple(r) for r in opt.x_vector.tolist()}) == 17
    np.random.seed(42)                             # a batch above BO_MAX_TOPQ: the rounds of select_indices
    big = B.BayesianOptimization(toy5, BOUNDS, n_objectives=5, initial_samples=8, n_iterations=1, batch_size=50,
                                 acquisition="mes", mes_samples=2, ts_features=64)
    big.optimize()
    assert len({tuple(r) for r in big.x_vector.tolist()}) == 58


# --------------------------------------------------------------------------- ranks
def rccl_run(n_ranks, force):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    if force:
        env["BO_FORCE_COLLECTIVES"] = "1"
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node", str(n_ranks), "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join("tests", "helpers", "mes_rccl_loop.py"), ROOT]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    return [json.loads(ln[7:]) for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]


def test_loop_over_rccl_one_rank(bo):
    """One rank with BO_FORCE_COLLECTIVES=1: the maxima go through the all_reduce(MAX) and the records
    through the all_gather; the picks equal the run without a process group."""
    res = rccl_run(1, True)
    assert len(res) == 1 and res[0]["collectives"] is True
    assert res[0]["x"] == loop("mes").x_vector.tolist()


def test_loop_two_ranks(bo):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    res = rccl_run(2, False)
    want = loop("mes").x_vector.tolist()
    assert sorted(r["rank"] for r in res) == [0, 1]
    for r in res:
        assert r["collectives"] is True and r["x"] == want, r["rank"]

"""Thompson-sampling batches from pathwise posterior draws (bo_sample_paths, acquisition.sample_paths /
select_batch_ts, batch_strategy="ts") against the extended-precision reference of tests/ts_ref.py.

The weights v are checked under tol_v; the paths are checked under tol_z with the device's OWN v
(weights_out) as data, at every candidate, so the bound holds at any cond(K).  A different pick at draw
s changes what later draws may take, so the selection tests assert ON THE REFERENCE ALONE that the gap
between the picked value and the next unpicked one exceeds 10 tol at every pick (check_topq's criterion;
the seeds are chosen for it) and then require the device's picks to equal the reference's exactly.

The staged chunk of ts_paths_kernel is kChunkDoubles = 4096 doubles of rows and weights: 212 rows at
dim 2 and S <= 16; CHUNK_CASE has D = 300 and N = 230, so both the feature rows and the kernel rows take
more than one chunk."""
import functools
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import ts_ref as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG_OFFSET = (1 << 31) + 12345 * 65536 + 777      # tests/test_gpu_bucb.py: a 65536 x 65536 grid past 2^31
PVS = np.array([1.3, 0.7, 1.1, 0.9, 1.2, 0.8, 1.05, 0.6])


@pytest.fixture(scope="module")
def bo():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import bayesopt_smart_amd as bo
    return bo


# --------------------------------------------------------------------------- cases (numpy only)
def grid_points(lo, shape):
    ax = [np.arange(l, l + s) for l, s in zip(lo, shape)]
    return np.stack([m.ravel() for m in np.meshgrid(*ax, indexing="ij")], axis=-1).astype(np.float64)


def smooth_y(rng, x, n_obj, span):
    y = np.empty((x.shape[0], n_obj))
    for o in range(n_obj):
        w = rng.uniform(0.6, 1.6, x.shape[1]) * 2 * np.pi / span
        ph = rng.uniform(0, 2 * np.pi, x.shape[1])
        y[:, o] = np.sin(x * w + ph).sum(axis=1) + 0.05 * rng.standard_normal(x.shape[0])
    return y


def make_case(pts, x, seed, n_obj, ls, n_s, n_feat, lam=1e-6, span=None):
    from bayesopt_smart_amd.acquisition import thompson_draws
    rng = np.random.default_rng(seed + 1000)
    y = smooth_y(rng, x, n_obj, span or float(np.ptp(pts, axis=0).max()))
    pv = PVS[:n_obj]
    ls = np.resize(np.asarray(ls, dtype=np.float64), n_obj)
    kinv, cond = T.fitted_state(x, pv, ls, lam)
    draws = thompson_draws(np.random.default_rng(seed), n_obj, x.shape[1], x.shape[0], n_s, n_feat)
    return dict(pts=pts, x=x, y=y, pm=y.mean(axis=0), pv=pv, ls=ls, lam=lam, kinv=kinv, cond=cond, draws=draws)


@functools.lru_cache(maxsize=None)
def grid_case(n_feat, n_s, n=24, n_obj=2, ls=(4.0, 6.0), lam=1e-6, shape=(33, 31), seed=3):
    pts = grid_points((-5, 100), shape)
    rng = np.random.default_rng(seed)
    x = pts[rng.choice(pts.shape[0], n, replace=False)]
    return make_case(pts, x, seed, n_obj, ls, n_s, n_feat, lam)


@functools.lru_cache(maxsize=None)
def sobol_case():
    from scipy.stats import qmc
    pts = -2.0 + qmc.Sobol(6, scramble=False, bits=30).random(1 << 10) * 40.0
    x = np.random.default_rng(5).uniform(-2.0, 38.0, (40, 6))
    return make_case(pts, x, 5, 3, (14.0, 18.0, 16.0), 3, 64)


@functools.lru_cache(maxsize=None)
def shard_case():
    pts = grid_points((0, 0), (32, 32))
    x = pts[np.random.default_rng(11).choice(1024, 30, replace=False)]
    return make_case(pts, x, 11, 2, (4.0, 6.0), 5, 37)


@functools.lru_cache(maxsize=None)
def big_offset_case():
    row, col = divmod(BIG_OFFSET, 65536)
    pts = np.stack([np.full(1000, float(row)), col + np.arange(1000.0)], axis=1)
    rng = np.random.default_rng(16)
    x = np.concatenate([pts[rng.choice(1000, 20, replace=False)],
                        pts[rng.choice(1000, 10, replace=False)] + rng.choice([-6.0, 7.0], (10, 1)) * [1.0, 0.0]])
    return make_case(pts, x, 16, 2, (4.0, 6.0), 3, 37, span=300.0)


# --------------------------------------------------------------------------- device side
def cand_set(bo, case, kind, lo=None, shape=None):
    CS = bo.predict.CandidateSet
    if kind == "grid":
        return CS.grid([(l, l + s) for l, s in zip(lo, shape)])
    if kind == "i64":
        return CS.explicit(case["pts"].astype(np.int64), "cuda")
    if kind == "f64":
        return CS.explicit(case["pts"], "cuda")
    return CS.sobol_set(6, case["pts"].shape[0], lo=-2.0, scale=40.0, bits=30)


def run_paths(case, cands, offset=0, count=None, ld=None):
    """(z [S, n_obj, count], v [S, n_obj, N]) of the device call, as numpy."""
    from bayesopt_smart_amd.acquisition import sample_paths
    z, v = sample_paths(case["x"], case["y"], case["kinv"], cands, case["pm"], case["pv"], case["ls"],
                        case["draws"], offset=offset, count=count, jitter=case["lam"], ld=ld,
                        return_weights=True, device="cuda")
    return z.cpu().numpy(), v.cpu().numpy()


def check(case, z, v, pts=None, label=""):
    """The weights under tol_v, then the paths under tol_z with the device's own v as data."""
    pts = case["pts"] if pts is None else pts
    v_ref, tol_v = T.weights(case["x"], case["y"], case["pm"], case["pv"], case["ls"], case["lam"], case["draws"],
                             case["kinv"])
    rv = (np.abs(v - v_ref) / tol_v).max()
    ref = T.paths(case["x"], pts, case["pm"], case["pv"], case["ls"], case["draws"], v)
    rz = (np.abs(z[:, :, ref["sel"]] - ref["z"]) / ref["tol_z"]).max()
    print(f"{label} cond {case['cond'].max():.3g} |dv|/tol_v {rv:.3g} |dz|/tol_z {rz:.3g}")
    assert np.isfinite(z).all() and np.isfinite(v).all()
    assert rv <= 1.0, (label, "weights", rv)
    assert rz <= 1.0, (label, "paths", rz)


@pytest.mark.parametrize("n_s", [1, 3, 16, 17, 48])
@pytest.mark.parametrize("n_feat", [37, 256])
def test_paths_grid(bo, n_feat, n_s):
    case = grid_case(n_feat, n_s)
    z, v = run_paths(case, cand_set(bo, case, "grid", (-5, 100), (33, 31)))
    assert z.shape == (n_s, 2, 1023)
    check(case, z, v, label=f"grid D={n_feat} S={n_s}")


@pytest.mark.parametrize("kind", ["i64", "f64"])
def test_paths_explicit_kinds(bo, kind):
    case = grid_case(37, 3)
    z, v = run_paths(case, cand_set(bo, case, kind))
    check(case, z, v, label=kind)
    zg, vg = run_paths(case, cand_set(bo, case, "grid", (-5, 100), (33, 31)))
    assert np.array_equal(z, zg) and np.array_equal(v, vg)       # integer coordinates: the same bits


def test_paths_sobol(bo):
    case = sobol_case()
    z, v = run_paths(case, cand_set(bo, case, "sobol"))
    check(case, z, v, label="sobol 6-D")


@pytest.mark.parametrize("n_obj", [1, 8])
def test_paths_objective_counts(bo, n_obj):
    case = grid_case(37, 3, n_obj=n_obj, ls=(4.0, 6.0, 5.0, 7.0, 4.5, 6.5, 5.5, 8.0)[:n_obj])
    z, v = run_paths(case, cand_set(bo, case, "grid", (-5, 100), (33, 31)))
    check(case, z, v, label=f"n_obj={n_obj}")


def test_paths_one_training_point(bo):
    case = grid_case(37, 3, n=1)
    z, v = run_paths(case, cand_set(bo, case, "grid", (-5, 100), (33, 31)))
    check(case, z, v, label="N=1")


def test_paths_more_rows_than_a_chunk(bo):
    case = grid_case(300, 3, n=230, shape=(20, 15), ls=(2.0, 2.5))     # CHUNK_CASE: 300 candidates
    assert case["pts"].shape[0] == 300
    z, v = run_paths(case, cand_set(bo, case, "grid", (-5, 100), (20, 15)))
    check(case, z, v, label="D=300 N=230")


def test_paths_ill_conditioned(bo):
    """cond(K + lam I) > 1e12: only the bound makes the comparison meaningful."""
    case = grid_case(37, 3, ls=(40.0, 50.0), lam=1e-14)
    assert case["cond"].min() > 1e12, case["cond"]
    z, v = run_paths(case, cand_set(bo, case, "grid", (-5, 100), (33, 31)))
    check(case, z, v, label="ill-conditioned")


def test_shard_bits_equal_the_whole_call(bo):
    case = shard_case()
    cands = cand_set(bo, case, "grid", (0, 0), (32, 32))
    z, v = run_paths(case, cands)
    zs, vs = run_paths(case, cands, offset=512, count=400)
    assert zs.shape == (5, 2, 400)
    assert np.array_equal(zs, z[:, :, 512:912]) and np.array_equal(vs, v)
    check(case, z, v, label="32x32")


def test_offset_past_2_31(bo):
    case = big_offset_case()
    cands = bo.predict.CandidateSet.grid([(0, 65536), (0, 65536)])
    z, v = run_paths(case, cands, offset=BIG_OFFSET, count=1000)
    check(case, z, v, label="big offset")


def test_training_point_identity_on_the_device(bo):
    """Candidates = the training points (kind F64): f(x_n) = y_n - sqrt(lam) E_n - lam v_n."""
    case = grid_case(256, 3)
    cands = bo.predict.CandidateSet.explicit(case["x"], "cuda")
    z, v = run_paths(case, cands)
    ref = T.paths(case["x"], case["x"], case["pm"], case["pv"], case["ls"], case["draws"], v)
    eps = case["draws"][3]
    f = case["pm"][None, :, None] + np.sqrt(case["pv"])[None, :, None] * z
    want = case["y"].T[None] - np.sqrt(case["lam"]) * eps - case["lam"] * v
    sel = ref["sel"]
    tol = ref["tol_f"] + 2 * T.U * np.abs(f[:, :, sel])
    ratio = (np.abs(f[:, :, sel] - want[:, :, sel]) / tol).max()
    print("training-point identity: |f - (y - sqrt(lam) E - lam v)| / tol", ratio)
    assert ratio <= 1.0


def test_deterministic_and_independent_of_ld(bo):
    import torch
    from bayesopt_smart_amd.device import Workspace
    case = grid_case(37, 17)
    cands = cand_set(bo, case, "grid", (-5, 100), (33, 31))
    z0, v0 = run_paths(case, cands)
    Workspace.get(1, torch.device("cuda", torch.cuda.current_device())).fill_(255)
    z1, v1 = run_paths(case, cands)
    z2, v2 = run_paths(case, cands, ld=1200)
    assert np.array_equal(z0, z1) and np.array_equal(v0, v1)
    assert np.array_equal(z0, z2) and np.array_equal(v0, v2)


# --------------------------------------------------------------------------- selection
def pareto(y):
    keep = [not any((o >= p).all() and (o > p).any() for o in y) for p in y]
    return y[np.array(keep)]


def select_setup(case, kind):
    """(front, ref_point, reference acquisition [S, M], its tolerance [S, M]) with the reference's own v."""
    ref = T.reference(case["x"], case["y"], case["pts"], case["pm"], case["pv"], case["ls"], case["lam"],
                      case["draws"], case["kinv"], full=True)
    n_obj = len(case["pv"])
    tol_z = ref["tol_z"].copy()
    for o in range(n_obj):                                         # the weights' own error, through k
        k = T.rbf(case["pts"], case["x"], case["pv"][o], case["ls"][o])
        tol_z[:, o] += ref["tol_v"][:, o] @ k.T / np.sqrt(case["pv"][o])
    front, rp = pareto(case["y"]), case["y"].min(axis=0) - 1.0
    acq = T.acquisition(ref["z"], case["pm"], case["pv"], kind, front, rp)
    if kind == "sum_ucb":
        tol = tol_z.sum(axis=1) + n_obj * T.U * np.abs(ref["z"]).sum(axis=1)
    else:
        # HVI is a sum of products of clipped differences p_k - l_k: each factor errs by the draw's own
        # error and a few roundings; a product of extents bounds the other factors
        p = case["pm"][None, :, None] + np.sqrt(case["pv"])[None, :, None] * ref["z"]
        ext = np.abs(p - rp[None, :, None]) + 1.0
        dp = np.sqrt(case["pv"])[None, :, None] * tol_z + 4 * T.U * (np.abs(p) + np.abs(rp)[None, :, None])
        tol = sum(dp[:, k] * np.prod(np.delete(ext, k, axis=1), axis=1) for k in range(n_obj))
        # the last term: the box sum's roundings, and this reference's own inclusion-exclusion sum
        tol = tol + (64 * (len(front) + 1) + 2.0 ** len(front)) * T.U * np.prod(ext, axis=1)
    return front, rp, acq, tol


def run_select(case, cands, kind, excluded_pts, offset=0, count=None, **kw):
    from bayesopt_smart_amd.acquisition import select_batch_ts
    front_args = {}
    if kind == "hvi":
        front_args = dict(y_evaluated=case["y"], reference_point=case["y"].min(axis=0) - 1.0)
    return select_batch_ts(case["x"], case["y"], case["kinv"], cands, case["pm"], case["pv"], case["ls"],
                           case["draws"], excluded_pts, case["draws"][2].shape[0], acquisition=kind,
                           offset=offset, count=count, jitter=case["lam"], return_details=True, **front_args, **kw)


def assert_gaps(picks, vals, gaps, tol, what):
    for s, (p, v, g) in enumerate(zip(picks, vals, gaps)):
        if p >= 0:
            assert g > 10 * tol[s, p], (what, s, g, tol[s, p])


@pytest.mark.parametrize("kind,n_obj", [("sum_ucb", 2), ("sum_ucb", 3), ("hvi", 2), ("hvi", 3)])
def test_selection_equals_the_reference(bo, kind, n_obj):
    case = grid_case(64, 5, n=12, n_obj=n_obj, ls=(4.0, 6.0, 5.0)[:n_obj], seed=21)
    front, rp, acq, tol = select_setup(case, kind)
    excluded = (case["pts"][:, None, :] == case["x"][None, :, :]).all(-1).any(-1)
    picks, vals, gaps = T.select(acq, excluded)
    print(kind, n_obj, "gaps", gaps, "tol", [tol[s, p] for s, p in enumerate(picks)], "vals", vals)
    assert_gaps(picks, vals, gaps, tol, kind)
    if kind == "hvi":
        assert (vals > 0).all()                                    # a positive best HVI for every draw
    got = run_select(case, cand_set(bo, case, "grid", (-5, 100), (33, 31)), kind, case["x"])
    assert got["picks"].tolist() == picks.tolist()
    assert not excluded[got["picks"]].any()                        # evaluated points are never picked
    assert len(set(got["picks"].tolist())) == len(picks)           # no index twice


def test_equal_draws_take_the_next_best(bo):
    case = dict(grid_case(64, 4, n=12, seed=21))
    z, b, theta, eps = (a.copy() for a in case["draws"])
    theta[1], eps[1] = theta[0], eps[0]
    case["draws"] = (z, b, theta, eps)
    _, _, acq, tol = select_setup(case, "sum_ucb")
    excluded = (case["pts"][:, None, :] == case["x"][None, :, :]).all(-1).any(-1)
    picks, vals, gaps = T.select(acq, excluded)
    assert_gaps(picks, vals, gaps, tol, "equal draws")
    order = np.argsort(-np.where(excluded, -np.inf, acq[0]), kind="stable")
    assert picks[0] == order[0] and picks[1] == order[1]          # the later draw takes its next best
    got = run_select(case, cand_set(bo, case, "grid", (-5, 100), (33, 31)), "sum_ucb", case["x"])
    assert got["picks"].tolist() == picks.tolist()


def test_shard_with_fewer_candidates_than_draws(bo):
    case = grid_case(64, 5, n=12, seed=21)
    cands = cand_set(bo, case, "grid", (-5, 100), (33, 31))
    evaluated = np.concatenate([case["x"], case["pts"][101:102]])
    free = [i for i in (100, 101, 102) if not (case["pts"][i] == evaluated).all(-1).any()]
    assert 1 <= len(free) <= 2
    got = run_select(case, cands, "sum_ucb", evaluated, offset=100, count=3)
    picks = got["picks"]
    assert sorted(picks[:len(free)].tolist()) == free and (picks[len(free):] == -1).all()


def test_two_shards_merge_to_the_single_call(bo):
    from bayesopt_smart_amd.acquisition import resolve_ts_picks
    from bayesopt_smart_amd.predict import merge_topq
    case = grid_case(64, 5, n=12, seed=21)
    cands = cand_set(bo, case, "grid", (-5, 100), (33, 31))
    for kind in ("sum_ucb", "hvi"):
        whole = run_select(case, cands, kind, case["x"])
        a = run_select(case, cands, kind, case["x"], offset=0, count=500)
        b = run_select(case, cands, kind, case["x"], offset=500, count=523)
        lists = [merge_topq(np.stack([a["vals"][s], b["vals"][s]]),
                            np.stack([a["lists"][s], b["lists"][s]]), s + 1)[1] for s in range(5)]
        assert resolve_ts_picks(lists).tolist() == whole["picks"].tolist()


# --------------------------------------------------------------------------- the loop
def toy(x):
    return np.array([-((x[0] - 12) ** 2) / 50.0 + 3.0, -((x[1] - 118) ** 2) / 40.0 + 2.0 + 0.02 * x[0]])


def loop(bo, acquisition, ts_seed, record=None, float_type=None):
    from bayesopt_smart_amd import bayesian_optimization as B
    np.random.seed(42)
    opt = B.BayesianOptimization(toy, [(-5, 28), (100, 131)], n_objectives=2, initial_samples=8, n_iterations=2,
                                 batch_size=4, betas=np.array([2.0, 2.0]), acquisition=acquisition,
                                 batch_strategy="ts", ts_features=128, ts_seed=ts_seed,
                                 reference_point=[-30.0, -30.0], float_type=float_type)
    if record is not None:
        inner = opt._backend.select

        def spy(fitted, pm, pv, ls, betas, batch_size, evaluated, *a, **k):
            idx = inner(fitted, pm, pv, ls, betas, batch_size, evaluated, *a, **k)
            xd, yd, kinv = fitted
            record.append(dict(x=xd.cpu().numpy(), y=yd.cpu().numpy(), kinv=kinv.cpu().numpy(),
                               pm=np.array(pm, dtype=np.float64), pv=np.array(pv, dtype=np.float64),
                               ls=np.array(ls, dtype=np.float64), evaluated=np.array(evaluated, dtype=np.float64),
                               idx=np.array(idx)))
            return idx
        opt._backend.select = spy
    opt.optimize()
    return opt


@pytest.mark.parametrize("acquisition", ["sum_ucb", "hvi"])
def test_loop_picks(bo, acquisition):
    from bayesopt_smart_amd.acquisition import thompson_draws
    rec = []
    opt = loop(bo, acquisition, 7, rec)
    pts = grid_points((-5, 100), (33, 31))
    xs = opt.x_vector                     # every row: n_evaluations keeps the reference's count quirk
    print("x_vector", xs.tolist(), "picks", [it["idx"].tolist() for it in rec])
    assert len({tuple(r) for r in xs.tolist()}) == len(xs) == 16          # distinct, none evaluated twice
    rng = np.random.default_rng(7)                                          # the backend's generator
    for it in rec:
        draws = thompson_draws(rng, 2, 2, it["x"].shape[0], 4, 128)
        case = dict(pts=pts, x=it["x"], y=it["y"], pm=it["pm"], pv=it["pv"], ls=it["ls"], lam=1e-6,
                    kinv=it["kinv"], draws=draws)
        ref = T.reference(case["x"], case["y"], pts, case["pm"], case["pv"], case["ls"], 1e-6, draws, case["kinv"],
                          full=True)
        front, rp = pareto(it["y"]), np.array([-30.0, -30.0])
        acq = T.acquisition(ref["z"], case["pm"], case["pv"], acquisition, front, rp)
        excluded = (pts[:, None, :] == it["evaluated"][None, :, :]).all(-1).any(-1)
        picks, vals, gaps = T.select(acq, excluded)
        print(acquisition, "gaps", gaps, "vals", vals)
        assert (gaps > 1e-9).all()
        assert it["idx"].tolist() == picks.tolist()
    again = loop(bo, acquisition, 7)
    other = loop(bo, acquisition, 8)
    assert np.array_equal(again.x_vector, opt.x_vector)
    assert not np.array_equal(other.x_vector, opt.x_vector)


def test_loop_float32_branch_runs(bo):
    opt = loop(bo, "sum_ucb", 7, float_type=np.float32)
    xs = opt.x_vector                     # every row: n_evaluations keeps the reference's count quirk
    assert len({tuple(r) for r in xs.tolist()}) == len(xs) == 16


def test_loop_over_rccl_one_rank():
    """tests/test_gpu_rccl_one_rank.py's pattern: one rank, BO_FORCE_COLLECTIVES=1, so every draw's
    record block goes through the all_gather; the picks equal the run without a process group."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, BO_FORCE_COLLECTIVES="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join("tests", "helpers", "ts_rccl_loop.py"), ROOT]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    res = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])
    assert res["collectives"] is True and res["collectives_after"] is False
    for kind in ("sum_ucb", "hvi"):
        assert res["rccl"][kind] == res["plain"][kind]


def test_graph_replay_equals_the_direct_call(bo):
    """bo_sample_paths captured on a side stream and replayed twice over a workspace of 0xFF bytes
    (tests/test_gpu_bucb.py's pattern): nothing is left in the workspace from one call to the next."""
    import ctypes
    import torch
    from bayesopt_smart_amd import _lib
    case = grid_case(37, 17)
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    keep = [torch.as_tensor(np.ascontiguousarray(a), device=dev)
            for a in (case["x"], case["y"], case["kinv"]) + tuple(case["draws"])]
    x, y, kinv, z, b, theta, eps = keep
    d = _lib.TsDesc()
    d.n_obj, d.dim, d.n_train = 2, 2, x.shape[0]
    d.x_train, d.y, d.ld_y, d.kinv, d.ld_k = x.data_ptr(), y.data_ptr(), 2, kinv.data_ptr(), x.shape[0]
    d.cand_kind, d.n_samples, d.n_features, d.n_cand, d.ld = _lib.CAND_GRID, 17, 37, 1023, 1023
    for k, (lo, sh) in enumerate(zip((-5, 100), (33, 31))):
        d.grid_lo[k], d.grid_shape[k] = lo, sh
    for o in range(2):
        d.prior_mean[o], d.prior_var[o], d.length_scale[o] = case["pm"][o], case["pv"][o], case["ls"][o]
    d.jitter = case["lam"]
    d.z, d.phase, d.theta, d.eps = z.data_ptr(), b.data_ptr(), theta.data_ptr(), eps.data_ptr()
    paths = torch.zeros((17, 2, 1023), dtype=torch.float64, device=dev)
    wts = torch.zeros((17, 2, x.shape[0]), dtype=torch.float64, device=dev)
    d.paths, d.weights_out = paths.data_ptr(), wts.data_ptr()
    ws = torch.empty(lib.bo_sample_paths_workspace_size(ctypes.byref(d)), dtype=torch.uint8, device=dev)
    assert lib.bo_sample_paths(ctypes.byref(d), None, 0, None) == _lib.ERR_WORKSPACE
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.bo_sample_paths(ctypes.byref(d), ws.data_ptr(), ws.numel(), stream) == 0
    direct = (paths.cpu().numpy().copy(), wts.cpu().numpy().copy())
    zr, vr = run_paths(case, cand_set(bo, case, "grid", (-5, 100), (33, 31)))
    assert np.array_equal(direct[0], zr) and np.array_equal(direct[1], vr)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side, capture_error_mode="relaxed"):
            assert lib.bo_sample_paths(ctypes.byref(d), ws.data_ptr(), ws.numel(), side.cuda_stream) == 0
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        ws.fill_(0xFF)
        paths.zero_()
        wts.zero_()
        g.replay()
        assert np.array_equal(paths.cpu().numpy(), direct[0]) and np.array_equal(wts.cpu().numpy(), direct[1])

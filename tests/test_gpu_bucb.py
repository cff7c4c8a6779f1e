"""Batch selection by hallucinated observations (bo_select_batch_bucb, acquisition.select_batch_bucb,
batch_strategy="bucb") against the numpy reference of tests/bucb_ref.py: the posterior variance of
a GP trained on X u {picks}, from the inverse of the augmented Gram matrix.

Tolerances are tests/parity.py's rule: var within 1e-5 pv, acq within 1e-5 max(1, |ref|).  Every
case asserts cond(K + jitter I) < 1e6 (the regime that rule is stated for).  A different pick at
step t changes every later step, so the selection tests assert ON THE REFERENCE ALONE that the
best-to-second gap of acq_t exceeds 10 tol at every step (check_topq's criterion; the seeds are
chosen for it) and then require the device's indices to equal the reference's exactly.

The device call gets std_mu / var / kinv computed by numpy (the call is tested in isolation);
the loop test runs the whole pipeline.
"""
import ctypes
import functools

import numpy as np
import pytest

import bucb_ref as R

pytestmark = pytest.mark.gpu

TOL = R.RTOL


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


def make_case(pts, x, seed, n_obj, ls, q, jitter=1e-6, min_var=1e-10, excluded=None, sl=None, span=None):
    """Reference batch over pts[sl] (the shard) for training points x; excluded over ALL pts."""
    rng = np.random.default_rng(seed + 1000)
    span = span or float(np.ptp(pts, axis=0).max())
    y = smooth_y(rng, x, n_obj, span)
    pm = y.mean(axis=0)
    pv = np.array([1.3, 0.7, 1.1, 0.9][:n_obj])
    beta = np.full(n_obj, 2.0)
    ls = np.asarray(ls, dtype=np.float64)[:n_obj]
    kinv, cond = R.fitted_state(x, y, pm, pv, ls, jitter)
    assert cond.max() < 1e6, cond                      # the conditioning rule of the f64 tolerances
    sl = sl or slice(0, pts.shape[0])
    if excluded is None:
        excluded = (pts[:, None, :] == x[None, :, :]).all(-1).any(-1)
    ref = R.bucb_reference(x, y, pts[sl], pm, pv, ls, beta, jitter, min_var, q, excluded[sl])
    return dict(pts=pts, x=x, y=y, pm=pm, pv=pv, ls=ls, beta=beta, jitter=jitter, min_var=min_var, kinv=kinv,
                q=q, excluded=excluded, offset=sl.start, count=sl.stop - sl.start, ref=ref)


def assert_gaps(ref):
    """The selection precondition, on the reference alone."""
    for t, (p, v, g) in enumerate(zip(ref["idx"], ref["val"], ref["gaps"])):
        if p >= 0:
            assert g > 10 * TOL * max(1.0, abs(v)), (t, g, v)


@functools.lru_cache(maxsize=None)
def grid_case(n, seed, q=5, shape=(33, 31), lo=(-5, 100), n_obj=2, ls=(4.0, 6.0), jitter=1e-6, min_var=1e-10):
    pts = grid_points(lo, shape)
    rng = np.random.default_rng(seed)
    x = pts[rng.choice(pts.shape[0], n, replace=False)]
    return make_case(pts, x, seed, n_obj, ls, q, jitter, min_var)


@functools.lru_cache(maxsize=None)
def sobol_case():
    from scipy.stats import qmc
    pts = -2.0 + qmc.Sobol(6, scramble=False, bits=30).random(1 << 10) * 40.0
    rng = np.random.default_rng(5)
    x = rng.uniform(-2.0, 38.0, (40, 6))
    return make_case(pts, x, 5, 3, (14.0, 18.0, 16.0), 4)


@functools.lru_cache(maxsize=None)
def shard_case():
    pts = grid_points((0, 0), (32, 32))
    rng = np.random.default_rng(11)
    x = pts[rng.choice(1024, 30, replace=False)]
    return make_case(pts, x, 11, 2, (4.0, 6.0), 5, sl=slice(512, 912))


BIG_OFFSET = (1 << 31) + 12345 * 65536 + 777      # a shard of a 65536 x 65536 grid past index 2^31


@functools.lru_cache(maxsize=None)
def big_offset_case():
    """1000 consecutive candidates of one grid row whose global indices exceed 2^31 (the 64-bit
    index decode); the training points: 20 of them and 10 on the neighbouring rows."""
    row, col = divmod(BIG_OFFSET, 65536)
    pts = np.stack([np.full(1000, float(row)), col + np.arange(1000.0)], axis=1)
    rng = np.random.default_rng(16)          # a design without ties on the plateau far from the data
    x = np.concatenate([pts[rng.choice(1000, 20, replace=False)],
                        pts[rng.choice(1000, 10, replace=False)] + rng.choice([-6.0, 7.0], (10, 1)) * [1.0, 0.0]])
    case = make_case(pts, x, 16, 2, (4.0, 6.0), 5, span=300.0)
    case["offset"] = BIG_OFFSET
    return case


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


def evaluated_of(case):
    """Points whose mask bits are the case's `excluded` (rows of pts)."""
    return case["pts"][case["excluded"]]


def run(bo, case, cands, q=None, **kw):
    import torch
    from bayesopt_smart_amd.acquisition import select_batch_bucb
    ref = case["ref"]
    smu = torch.as_tensor(np.ascontiguousarray(ref["smu"]), device="cuda")
    var = torch.as_tensor(np.ascontiguousarray(ref["var0"]), device="cuda")
    keep = (smu.clone(), var.clone())
    res = select_batch_bucb(smu, var, case["x"], case["kinv"], cands, case["pv"], case["ls"], case["beta"],
                            evaluated_of(case), q or case["q"], offset=case["offset"], count=case["count"],
                            jitter=case["jitter"], min_variance=case["min_var"], return_details=True, **kw)
    out = {k: v.cpu().numpy() for k, v in res.items()}
    assert torch.equal(smu, keep[0]) and torch.equal(var, keep[1]), "the inputs were modified"
    return out


def check_parity(case, got, ref=None):
    ref = ref or case["ref"]
    want = np.where(ref["idx"] >= 0, ref["idx"] + case["offset"], -1)
    print("idx", got["top_idx"], "ref", want, "min gap", ref["gaps"].min(),
          "max |dvar|/pv", (np.abs(got["var"] - ref["var"]) / case["pv"][:, None]).max(),
          "max |dacq|", np.abs(got["acq"] - ref["acq"]).max())
    np.testing.assert_array_equal(got["top_idx"], want)
    ok = ref["idx"] >= 0
    assert np.all(np.abs(got["top_val"][ok] - ref["val"][ok]) <= TOL * np.maximum(1.0, np.abs(ref["val"][ok])))
    assert np.all(np.isneginf(got["top_val"][~ok]))
    assert np.all(np.abs(got["var"] - ref["var"]) <= TOL * case["pv"][:, None])
    assert np.all(np.abs(got["acq"] - ref["acq"]) <= TOL * np.maximum(1.0, np.abs(ref["acq"])))


# 1. parity on a grid with a ragged last workgroup and wave: 33 x 31 = 1023 candidates
@pytest.mark.parametrize("n,seed", [(24, 1), (37, 2)])
def test_parity_grid(bo, n, seed):
    case = grid_case(n, seed)
    assert_gaps(case["ref"])
    got = run(bo, case, cand_set(bo, case, "grid", (-5, 100), (33, 31)))
    check_parity(case, got)
    assert len(set(got["top_idx"])) == 5 and not case["excluded"][got["top_idx"]].any()


# 2. q = 1 is today's selection
def test_q1_is_the_masked_top1(bo):
    import torch
    from bayesopt_smart_amd.acquisition import ExclusionMask, select_indices
    case = grid_case(24, 1)
    cands = cand_set(bo, case, "grid", (-5, 100), (33, 31))
    got = run(bo, case, cands, q=1)
    acq1 = R.acquisition(case["ref"]["smu"], case["ref"]["var0"], case["pv"], case["beta"])
    mask = ExclusionMask(cands, 0, cands.n, "cuda").update(evaluated_of(case))
    top1 = select_indices(torch.as_tensor(acq1, device="cuda"), cands, evaluated_of(case), 1, mask=mask)
    assert got["top_idx"].tolist() == top1.tolist() == [case["ref"]["idx"][0]]
    # acq_out is the acquisition that pick was taken from; var_out the variance after that one pick
    assert np.all(np.abs(got["acq"] - acq1) <= TOL * np.maximum(1.0, np.abs(acq1)))
    one = R.bucb_reference(case["x"], case["y"], case["pts"], case["pm"], case["pv"], case["ls"], case["beta"],
                           case["jitter"], case["min_var"], 1, case["excluded"])
    assert np.all(np.abs(got["var"] - one["var"]) <= TOL * case["pv"][:, None])
    assert (got["var"] < case["ref"]["var0"] - 1e-3).any()        # it is not the input variance


# 3. the candidate kinds agree
def test_kinds_agree_grid_i64_f64(bo):
    case = grid_case(24, 1)
    g = run(bo, case, cand_set(bo, case, "grid", (-5, 100), (33, 31)))
    i = run(bo, case, cand_set(bo, case, "i64"))
    f = run(bo, case, cand_set(bo, case, "f64"))
    np.testing.assert_array_equal(g["top_idx"], i["top_idx"])
    np.testing.assert_array_equal(g["top_idx"], f["top_idx"])
    assert i["var"].tobytes() == f["var"].tobytes()
    check_parity(case, f)


def test_kinds_agree_sobol_f64_6d(bo):
    case = sobol_case()
    assert_gaps(case["ref"])
    s = run(bo, case, cand_set(bo, case, "sobol"))
    f = run(bo, case, cand_set(bo, case, "f64"))
    np.testing.assert_array_equal(s["top_idx"], f["top_idx"])
    check_parity(case, s)
    check_parity(case, f)


def test_one_objective(bo):
    case = grid_case(24, 3, n_obj=1, ls=(5.0,))
    assert_gaps(case["ref"])
    check_parity(case, run(bo, case, cand_set(bo, case, "grid", (-5, 100), (33, 31))))


# 4. a shard: cand_offset 512, 400 of 1024 candidates
@pytest.mark.parametrize("kind", ["grid", "f64"])
def test_shard(bo, kind):
    case = shard_case()
    assert_gaps(case["ref"])
    got = run(bo, case, cand_set(bo, case, kind, (0, 0), (32, 32)))
    assert np.all((got["top_idx"] >= 512) & (got["top_idx"] < 912))
    check_parity(case, got)


def test_shard_past_2_31(bo):
    """Global indices past 2^31: the 64-bit grid decode, and top_idx beyond int32."""
    case = big_offset_case()
    assert_gaps(case["ref"])
    got = run(bo, case, cand_set(bo, case, "grid", (0, 0), (65536, 65536)))
    assert got["top_idx"].min() >= BIG_OFFSET > (1 << 31)
    check_parity(case, got)


# 5. exclusion and no repeats
def test_masked_argmax_is_never_returned(bo):
    base = grid_case(24, 1)
    top = base["ref"]["idx"][0]
    excluded = base["excluded"].copy()
    excluded[top] = True
    case = make_case(base["pts"], base["x"], 1, 2, (4.0, 6.0), 5, excluded=excluded)
    assert_gaps(case["ref"])
    got = run(bo, case, cand_set(bo, case, "grid", (-5, 100), (33, 31)))
    assert top not in got["top_idx"] and len(set(got["top_idx"])) == 5
    check_parity(case, got)


def test_fewer_candidates_than_q(bo):
    base = grid_case(24, 1)
    excluded = np.ones(base["pts"].shape[0], dtype=bool)
    excluded[[40, 500, 1022]] = False                    # 1022: the last candidate of the ragged wave
    case = make_case(base["pts"], base["x"], 1, 2, (4.0, 6.0), 5, excluded=excluded)
    assert_gaps(case["ref"])
    got = run(bo, case, cand_set(bo, case, "grid", (-5, 100), (33, 31)))
    assert sorted(got["top_idx"][:3]) == [40, 500, 1022] and got["top_idx"][3:].tolist() == [-1, -1]
    check_parity(case, got)


# 6. the largest q.  No gap precondition here: over 48 steps on 256 candidates near-ties are certain, so the
# reference is conditioned on the device's own picks and only the variance is compared.
def test_largest_q(bo):
    case = grid_case(12, 4, q=1, shape=(16, 16), lo=(0, 0))
    got = run(bo, case, cand_set(bo, case, "grid", (0, 0), (16, 16)), q=48)
    idx = got["top_idx"]
    assert len(set(idx)) == 48 and idx.min() >= 0 and not case["excluded"][idx].any()
    ref = R.bucb_reference(case["x"], case["y"], case["pts"], case["pm"], case["pv"], case["ls"], case["beta"],
                           case["jitter"], case["min_var"], 48, case["excluded"], picks=idx)
    print("max |dvar|/pv", (np.abs(got["var"] - ref["var"]) / case["pv"][:, None]).max())
    assert np.all(np.abs(got["var"] - ref["var"]) <= TOL * case["pv"][:, None])
    assert np.all(np.abs(got["top_val"] - ref["val"]) <= TOL * np.maximum(1.0, np.abs(ref["val"])))


# 7. the float32 branch's constants
def test_float32_branch_constants(bo):
    case = grid_case(24, 1, jitter=1e-3, min_var=1e-6)
    assert_gaps(case["ref"])
    got = run(bo, case, cand_set(bo, case, "grid", (-5, 100), (33, 31)))
    check_parity(case, got)
    assert got["var"].min() >= 1e-6
    # a floor that bites (above the variance left at the data and the picks, ~ jitter)
    hi = grid_case(24, 1, jitter=1e-3, min_var=5e-3)
    assert_gaps(hi["ref"])
    got = run(bo, hi, cand_set(bo, hi, "grid", (-5, 100), (33, 31)))
    check_parity(hi, got)
    assert got["var"].min() == 5e-3 and (got["var"] == 5e-3).sum() >= 24


# 8. / 9. graph replay over a garbage workspace, and determinism (raw ABI calls)
def raw_call(bo, case, ws=None):
    """(desc, outputs, keepalive, workspace) of a grid call through the C ABI."""
    import torch
    from bayesopt_smart_amd import _lib
    from bayesopt_smart_amd.acquisition import ExclusionMask
    lib = _lib.load()
    ref = case["ref"]
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")  # noqa: E731
    keep = dict(x=t(case["x"]), kinv=t(case["kinv"]), smu=t(ref["smu"]), var=t(ref["var0"]))
    cands = cand_set(bo, case, "grid", (-5, 100), (33, 31))
    keep["mask"] = ExclusionMask(cands, 0, cands.n, "cuda").update(evaluated_of(case))
    n_obj, m, q = len(case["pv"]), cands.n, case["q"]
    out = dict(top_val=torch.zeros(q, dtype=torch.float64, device="cuda"),
               top_idx=torch.zeros(q, dtype=torch.int64, device="cuda"),
               var=torch.zeros((n_obj, m), dtype=torch.float64, device="cuda"),
               acq=torch.zeros(m, dtype=torch.float64, device="cuda"))
    d = _lib.BucbDesc()
    d.n_obj, d.dim, d.n_train = n_obj, 2, case["x"].shape[0]
    d.x_train, d.kinv, d.ld_k = keep["x"].data_ptr(), keep["kinv"].data_ptr(), case["x"].shape[0]
    d.cand_kind, d.q, d.n_cand, d.cand_offset = _lib.CAND_GRID, q, m, 0
    for k in range(2):
        d.grid_lo[k], d.grid_shape[k] = (-5, 100)[k], (33, 31)[k]
    for o in range(n_obj):
        d.prior_var[o], d.length_scale[o], d.beta[o] = case["pv"][o], case["ls"][o], case["beta"][o]
    d.jitter, d.min_variance = case["jitter"], case["min_var"]
    d.std_mu, d.var, d.ld, d.mask = keep["smu"].data_ptr(), keep["var"].data_ptr(), m, keep["mask"].ptr
    d.top_val, d.top_idx = out["top_val"].data_ptr(), out["top_idx"].data_ptr()
    d.var_out, d.acq_out = out["var"].data_ptr(), out["acq"].data_ptr()
    nbytes = lib.bo_select_batch_bucb_workspace_size(ctypes.byref(d))
    assert nbytes > 0
    if ws is None:
        ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    return lib, d, out, keep, ws


def snapshot(out):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().tobytes() for k, v in out.items()}


def test_abi_status_codes(bo):
    from bayesopt_smart_amd import _lib
    lib, d, out, keep, ws = raw_call(bo, grid_case(24, 1))
    assert lib.bo_select_batch_bucb(ctypes.byref(d), ws.data_ptr(), ws.numel() - 256, None) == _lib.ERR_WORKSPACE
    assert lib.bo_select_batch_bucb(ctypes.byref(d), None, 0, None) == _lib.ERR_WORKSPACE
    d.ld = d.n_cand - 1
    assert lib.bo_select_batch_bucb(ctypes.byref(d), ws.data_ptr(), ws.numel(), None) == _lib.ERR_ARG
    d.ld = d.n_cand
    d.grid_shape[1] = 30                                  # the shard no longer fits the grid
    assert lib.bo_select_batch_bucb(ctypes.byref(d), ws.data_ptr(), ws.numel(), None) == _lib.ERR_ARG


def test_determinism_and_graph_replay(bo):
    import torch
    case = grid_case(24, 1)
    lib, d, out, keep, ws = raw_call(bo, case)
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.bo_select_batch_bucb(ctypes.byref(d), ws.data_ptr(), ws.numel(), stream) == 0
    direct = snapshot(out)
    np.testing.assert_array_equal(out["top_idx"].cpu().numpy(), case["ref"]["idx"])
    # 9. a second direct call: bit-identical
    for v in out.values():
        v.zero_()
    assert lib.bo_select_batch_bucb(ctypes.byref(d), ws.data_ptr(), ws.numel(), stream) == 0
    assert snapshot(out) == direct
    # 8. captured on a side stream, replayed twice over a workspace of 0xFF bytes: nothing is left
    # in the workspace from one call to the next
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side, capture_error_mode="relaxed"):
            assert lib.bo_select_batch_bucb(ctypes.byref(d), ws.data_ptr(), ws.numel(), side.cuda_stream) == 0
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        ws.fill_(0xFF)
        for v in out.values():
            v.zero_()
        g.replay()
        assert snapshot(out) == direct


# 10. the loop.  The fit is held at the given hyper-parameters (update_k + invert_k, no Powell): Powell
# on this quadratic drives cond(K + 1e-6 I) far past the 1e6 every case here keeps, where no two
# formulations agree on a pick.
LOOP_BOUNDS = [(118, 182), (118, 182)]
LOOP_LS = np.array([6.0, 5.0])
LOOP_PV = np.array([9.0e4, 8.0e4])


def toy_function(p):
    """examples/benchmark_functions.py:33-50 (2 objectives from x[0], x[1]), one point."""
    return np.array([-((p[0] - 150) ** 2) + 100, -((p[1] - 150) ** 2) + 20], dtype=np.float64)


def loop_initial_points():
    rng = np.random.default_rng(25)          # a design whose reference gaps hold in both iterations
    pts = grid_points((118, 118), (64, 64))
    return pts[rng.choice(pts.shape[0], 10, replace=False)]


def make_fixed_fit_backend(opt, states):
    import time
    import types

    import torch
    from bayesopt_smart_amd import kernels as K
    from bayesopt_smart_amd.bayesian_optimization import DeviceBackend

    class FixedFit(DeviceBackend):
        def fit(self, x_vector, y_vector, n, prior_mean, prior_variance, length_scales):
            xd = torch.as_tensor(np.ascontiguousarray(x_vector[:n], dtype=np.float64), device=self.dev)
            yd = torch.as_tensor(np.ascontiguousarray(y_vector[:n], dtype=np.float64), device=self.dev)
            K.update_k(self.bufs.kernel_matrices, xd, 0, n, prior_variance, length_scales)
            kinv = K.invert_k(n, self.bufs.kernel_matrices)
            return types.SimpleNamespace(x=np.concatenate([length_scales, prior_variance])), (xd, yd, kinv), \
                time.perf_counter()

        def select(self, *a, **kw):
            idx = DeviceBackend.select(self, *a, **kw)
            states.append((a[0][0].cpu().numpy().copy(), a[0][1].cpu().numpy().copy(), np.array(idx)))
            return idx

    return FixedFit(opt.candidates, 2, opt.total_samples, opt.device)


def run_loop(bo, states=None, **kw):
    opt = bo.BayesianOptimization(toy_function, LOOP_BOUNDS, n_objectives=2, n_iterations=2, batch_size=4,
                                  initial_points=loop_initial_points(), length_scales=LOOP_LS.copy(),
                                  prior_variance=LOOP_PV.copy(), betas=[2.0, 2.0], **kw)
    opt._backend = make_fixed_fit_backend(opt, [] if states is None else states)
    opt._buffers = opt._backend.bufs
    opt.optimize()
    return opt


def test_loop_bucb_matches_reference(bo):
    states = []
    opt = run_loop(bo, states, batch_strategy="bucb")
    assert len(states) == 2
    pts = grid_points((118, 118), (64, 64))
    for x, y, idx in states:
        excluded = (pts[:, None, :] == x[None, :, :]).all(-1).any(-1)
        _, cond = R.fitted_state(x, y, opt.prior_mean, LOOP_PV, LOOP_LS, 1e-6)
        assert cond.max() < 1e6, cond
        ref = R.bucb_reference(x, y, pts, opt.prior_mean, LOOP_PV, LOOP_LS, np.array([2.0, 2.0]), 1e-6, 1e-10, 4,
                               excluded)
        assert_gaps(ref)
        print("batch", idx, "ref", ref["idx"], "min gap", ref["gaps"].min())
        np.testing.assert_array_equal(idx, ref["idx"])
    np.testing.assert_array_equal(opt.x_vector[10:14], pts[states[0][2]])


def test_loop_top_is_the_default(bo):
    a = run_loop(bo)
    b = run_loop(bo, batch_strategy="top")
    np.testing.assert_array_equal(a.x_vector, b.x_vector)
    np.testing.assert_array_equal(a.y_vector, b.y_vector)

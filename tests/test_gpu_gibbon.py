"""GIBBON batches (bo_select_batch_gibbon, acquisition.select_batch_gibbon, batch_strategy="gibbon")
against the numpy reference of tests/gibbon_ref.py: the variance after t picks is the posterior
variance of a GP trained on X u {picks}, from the inverse of the augmented Gram matrix.

The device call gets `base` and `var` computed by numpy (the call is tested in isolation); `base` is
the max-value entropy over the maxima of exact joint posterior draws.  The loop test runs the whole
pipeline.

Three rules are checked.
  variance     |var_out - ref| <= 1e-5 pv (bucb_ref.RTOL, the project's rule)
  composition  acq_last against numpy's base + 0.5 sum_o log(var_dev / var0) from the DEVICE's own
               var_out of the run with one pick fewer, within
               (n_obj + 6) 2^-53 (|base| + sum_o |log r_o|) + 2^-1022 (gibbon_ref.compose)
  picks        equal to the reference's exactly, after asserting ON THE REFERENCE ALONE that at every
               pick the best candidate leads every other one by more than the two rules above can
               move them, with a tenfold margin on the variance rule (gibbon_ref.margin)
The margin cannot hold for a candidate next to a training point (var0 ~ 1e-6 pv: a relative
variance error of 1e-5 pv / var0 is unbounded there), so the cases' masks also exclude every
candidate within `radius` grid steps of a training point.  The seeds are the ones a CPU search over
1..8 with this file's own generator found to satisfy the margin.
"""
import ctypes
import functools

import numpy as np
import pytest

import bucb_ref as R
import gibbon_ref as G
import test_gpu_bucb as TB

pytestmark = pytest.mark.gpu

PV8 = np.array([1.3, 0.7, 1.1, 0.9, 1.2, 0.8, 1.0, 0.6])
LS8 = np.array([4.0, 6.0, 5.0, 7.0, 4.5, 5.5, 6.5, 5.0])


@pytest.fixture(scope="module")
def bo():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import bayesopt_smart_amd as bo
    return bo


# --------------------------------------------------------------------------- cases (numpy only)
def near_training(pts, x, radius):
    d2 = ((pts[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    return (d2 <= radius * radius).any(-1)


def make_case(pts, x, seed, n_obj, q, n_s=4, radius=1.5, pv=None, ls=None, jitter=1e-6, min_var=1e-10, sl=None,
              span=None, excluded=None):
    """Reference batch over pts[sl] (the shard) for training points x; `excluded` over ALL pts."""
    rng = np.random.default_rng(seed + 1000)
    span = span or float(np.ptp(pts, axis=0).max())
    y = TB.smooth_y(rng, x, n_obj, span)
    pm = y.mean(axis=0)
    pv = PV8[:n_obj] if pv is None else np.asarray(pv, dtype=np.float64)
    ls = LS8[:n_obj] if ls is None else np.asarray(ls, dtype=np.float64)
    kinv, cond = R.fitted_state(x, y, pm, pv, ls, jitter)
    assert cond.max() < 1e6, cond                      # the conditioning rule of the f64 tolerances
    sl = sl or slice(0, pts.shape[0])
    if excluded is None:
        excluded = near_training(pts, x, radius)
    # the single-point acquisition: the max-value entropy over the maxima of exact joint draws of
    # the posterior over ALL points
    mu, cov = G.posterior_mean_cov(x, y, pts, pm, pv, ls, jitter)
    var_all = np.maximum(np.einsum("oii->oi", cov), min_var)
    ystar = G.sampled_maxima(mu, cov, n_s, seed + 2000)
    base = G.mes(mu, var_all, ystar)[sl]
    ref = G.gibbon_reference(x, y, pts[sl], pm, pv, ls, jitter, min_var, q, excluded[sl], base)
    return dict(pts=pts, x=x, y=y, pm=pm, pv=pv, ls=ls, jitter=jitter, min_var=min_var, kinv=kinv, q=q,
                excluded=excluded, offset=sl.start, count=sl.stop - sl.start, base=base, mu=mu[:, sl], ystar=ystar,
                ref=ref)


GRID_LO, GRID_SHAPE = (-5, 100), (33, 31)
# n_obj -> (N, seed, S, radius, length scales): 1023 candidates, a ragged last workgroup and wave.
# The search (seeds 1..8, N = 24 and 37, S = 4) found no seed for 5 objectives with LS8[:5] at either
# N: with those scales the interior between the training points has var0 so small that the tenfold
# variance rule alone moves a candidate by more than the gaps.  With the shorter scales below, 5 of
# the 8 seeds pass at N = 37.
GRID_CASES = {1: (37, 5, 4, 1.5, None), 2: (24, 5, 4, 1.5, None), 3: (24, 1, 4, 1.5, None),
              5: (37, 8, 4, 1.5, (4.0, 4.5, 5.0, 4.2, 4.8)), 8: (37, 1, 4, 2.9, None)}


@functools.lru_cache(maxsize=None)
def grid_case(n_obj, q=5, jitter=1e-6, min_var=1e-10):
    n, seed, n_s, radius, ls = GRID_CASES[n_obj]
    pts = TB.grid_points(GRID_LO, GRID_SHAPE)
    rng = np.random.default_rng(seed)
    x = pts[rng.choice(pts.shape[0], n, replace=False)]
    return make_case(pts, x, seed, n_obj, q, n_s=n_s, radius=radius, ls=ls, jitter=jitter, min_var=min_var)


SOBOL_SEED, SOBOL_RADIUS = 5, 0.0        # no candidate of the Sobol set is near a training point


@functools.lru_cache(maxsize=None)
def sobol_case():
    from scipy.stats import qmc
    pts = -2.0 + qmc.Sobol(6, scramble=False, bits=30).random(1 << 10) * 40.0
    rng = np.random.default_rng(SOBOL_SEED)
    x = rng.uniform(-2.0, 38.0, (40, 6))
    return make_case(pts, x, SOBOL_SEED, 3, 4, radius=SOBOL_RADIUS, ls=(14.0, 18.0, 16.0))


SHARD_SEED = 2


@functools.lru_cache(maxsize=None)
def shard_case():
    pts = TB.grid_points((0, 0), (32, 32))
    rng = np.random.default_rng(SHARD_SEED)
    x = pts[rng.choice(1024, 30, replace=False)]
    return make_case(pts, x, SHARD_SEED, 2, 5, sl=slice(512, 912))


def assert_margins(ref):
    """The selection precondition, on the reference alone."""
    for t, (p, m) in enumerate(zip(ref["idx"], ref["margins"])):
        if p >= 0:
            assert m > 0.0, (t, p, m)


# --------------------------------------------------------------------------- device side
def grid_set(bo, case):
    return TB.cand_set(bo, case, "grid", GRID_LO, GRID_SHAPE)


def run(bo, case, cands, q=None, base=None, var0=None, mask=None, **kw):
    import torch
    from bayesopt_smart_amd.acquisition import select_batch_gibbon
    b = torch.as_tensor(np.ascontiguousarray(case["base"] if base is None else base), device="cuda")
    v = torch.as_tensor(np.ascontiguousarray(case["ref"]["var0"] if var0 is None else var0), device="cuda")
    keep = (b.clone(), v.clone())
    args = dict(jitter=case["jitter"], min_variance=case["min_var"])
    args.update(kw)
    res = select_batch_gibbon(b, v, case["x"], case["kinv"], cands, case["pv"], case["ls"], TB.evaluated_of(case),
                              q or case["q"], offset=case["offset"], count=case["count"], mask=mask,
                              return_details=True, **args)
    out = {k: t.cpu().numpy() for k, t in res.items()}
    same = lambda a, c: torch.equal(a.view(torch.int64), c.view(torch.int64))   # noqa: E731  (NaN-safe)
    assert same(b, keep[0]) and same(v, keep[1]), "the inputs were modified"
    return out


def check_parity(case, got, ref=None):
    """Rules `variance` and `picks` (the margins are asserted by the caller)."""
    ref = ref or case["ref"]
    want = np.where(ref["idx"] >= 0, ref["idx"] + case["offset"], -1)
    print("idx", got["top_idx"], "ref", want, "min margin", ref["margins"].min(),
          "max |dvar|/pv", (np.abs(got["var"] - ref["var"]) / case["pv"][:, None]).max())
    np.testing.assert_array_equal(got["top_idx"], want)
    assert np.all(np.abs(got["var"] - ref["var"]) <= G.RTOL * case["pv"][:, None])
    ok = ref["idx"] >= 0
    assert np.all(np.isneginf(got["top_val"][~ok]))
    # the values: the reference's within what the variance rule allows (the margin's E) -- loose on
    # purpose, the exact statement is the composition test's
    assert np.allclose(got["top_val"][ok], ref["val"][ok], rtol=0, atol=1e-3)


# 1. + 3. variance parity and the reference's picks
@pytest.mark.parametrize("n_obj", [1, 2, 3, 5, 8])
def test_parity_grid(bo, n_obj):
    case = grid_case(n_obj)
    assert_margins(case["ref"])
    got = run(bo, case, grid_set(bo, case))
    check_parity(case, got)
    assert len(set(got["top_idx"])) == 5 and not case["excluded"][got["top_idx"]].any()
    # the batch spreads: the reference's property, so the device's
    top = np.argsort(-np.where(case["excluded"], -np.inf, case["base"]), kind="stable")[:5]
    print("min distance of the batch", G.pairwise(case["pts"][got["top_idx"]])[0], "max distance of the top 5",
          G.pairwise(case["pts"][top])[1])


# 2. the exact composition, from the device's own variance
@pytest.mark.parametrize("n_obj", [1, 2, 3, 5, 8])
def test_exact_composition(bo, n_obj):
    case = grid_case(n_obj)
    cands = grid_set(bo, case)
    base, var0, excluded = case["base"], case["ref"]["var0"], case["excluded"]
    worst = 0.0
    for t in range(2, 6):
        prev = run(bo, case, cands, q=t - 1)
        got = run(bo, case, cands, q=t)
        np.testing.assert_array_equal(got["top_idx"][: t - 1], prev["top_idx"])
        want, bound = G.compose(base, prev["var"], var0)
        err = np.abs(got["acq_last"] - want)
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (t, float((err / bound).max()))
        avail = ~excluded
        avail[got["top_idx"][: t - 1]] = False
        p, _ = R.best(got["acq_last"], avail)                        # exact: the device's own array
        assert got["top_idx"][t - 1] == p
        assert got["top_val"][t - 1].tobytes() == got["acq_last"][p].tobytes()
    print(f"n_obj {n_obj}: worst |acq_last - numpy| / bound = {worst:.3g}")


# 4. q = 1 is the masked top-1 of base
def test_q1_is_the_masked_top1(bo):
    import torch
    from bayesopt_smart_amd.acquisition import ExclusionMask, select_indices
    case = grid_case(2)
    cands = grid_set(bo, case)
    got = run(bo, case, cands, q=1)
    mask = ExclusionMask(cands, 0, cands.n, "cuda").update(TB.evaluated_of(case))
    top1 = select_indices(torch.as_tensor(case["base"], device="cuda"), cands, TB.evaluated_of(case), 1, mask=mask)
    assert got["top_idx"].tolist() == top1.tolist() == [case["ref"]["idx"][0]]
    assert got["acq_last"].tobytes() == case["base"].tobytes()        # the first pass adds nothing
    assert got["top_val"][0] == case["base"][top1[0]]
    one = G.gibbon_reference(case["x"], case["y"], case["pts"], case["pm"], case["pv"], case["ls"], case["jitter"],
                             case["min_var"], 1, case["excluded"], case["base"])
    assert np.all(np.abs(got["var"] - one["var"]) <= G.RTOL * case["pv"][:, None])
    assert (got["var"] < case["ref"]["var0"] - 1e-3).any()            # it is not the input variance


# 5. the candidate kinds
def test_kinds_agree_grid_i64_f64(bo):
    case = grid_case(3)
    g = run(bo, case, grid_set(bo, case))
    i = run(bo, case, TB.cand_set(bo, case, "i64"))
    f = run(bo, case, TB.cand_set(bo, case, "f64"))
    for k in ("top_idx", "top_val", "var", "acq_last"):
        assert g[k].tobytes() == i[k].tobytes() == f[k].tobytes(), k


def test_kinds_agree_sobol_f64_6d(bo):
    case = sobol_case()
    assert not case["excluded"].any()
    assert_margins(case["ref"])
    f = run(bo, case, TB.cand_set(bo, case, "f64"))
    s = run(bo, case, TB.cand_set(bo, case, "sobol"))
    np.testing.assert_array_equal(s["top_idx"], f["top_idx"])
    check_parity(case, s)
    check_parity(case, f)


@pytest.mark.parametrize("kind", ["grid", "f64"])
def test_shard(bo, kind):
    case = shard_case()
    assert_margins(case["ref"])
    got = run(bo, case, TB.cand_set(bo, case, kind, (0, 0), (32, 32)))
    assert np.all((got["top_idx"] >= 512) & (got["top_idx"] < 912))
    check_parity(case, got)


# 6. edge cases
def test_masked_argmax_is_never_returned(bo):
    case = grid_case(2)
    top = case["ref"]["idx"][0]
    excluded = case["excluded"].copy()
    excluded[top] = True
    other = dict(case, excluded=excluded)
    got = run(bo, other, grid_set(bo, case))
    assert top not in got["top_idx"] and len(set(got["top_idx"])) == 5 and not excluded[got["top_idx"]].any()
    ref = G.gibbon_reference(case["x"], case["y"], case["pts"], case["pm"], case["pv"], case["ls"], case["jitter"],
                             case["min_var"], 5, excluded, case["base"], picks=got["top_idx"])
    assert np.all(np.abs(got["var"] - ref["var"]) <= G.RTOL * case["pv"][:, None])


def test_fewer_candidates_than_q(bo):
    case = grid_case(2)
    excluded = np.ones(case["pts"].shape[0], dtype=bool)
    excluded[[40, 500, 1022]] = False                    # 1022: the last candidate of the ragged wave
    got = run(bo, dict(case, excluded=excluded), grid_set(bo, case))
    assert sorted(got["top_idx"][:3]) == [40, 500, 1022] and got["top_idx"][3:].tolist() == [-1, -1]
    assert np.all(np.isfinite(got["top_val"][:3])) and np.all(np.isneginf(got["top_val"][3:]))


def test_largest_q(bo):
    """48 picks on 256 candidates: near-ties are certain, so the reference is conditioned on the
    device's own picks and only the variance is compared."""
    pts = TB.grid_points((0, 0), (16, 16))
    rng = np.random.default_rng(4)
    x = pts[rng.choice(256, 12, replace=False)]
    case = make_case(pts, x, 4, 2, 1, radius=0.0)
    got = run(bo, case, TB.cand_set(bo, case, "grid", (0, 0), (16, 16)), q=48)
    idx = got["top_idx"]
    assert len(set(idx)) == 48 and idx.min() >= 0 and not case["excluded"][idx].any()
    ref = G.gibbon_reference(case["x"], case["y"], pts, case["pm"], case["pv"], case["ls"], case["jitter"],
                             case["min_var"], 48, case["excluded"], case["base"], picks=idx)
    print("max |dvar|/pv", (np.abs(got["var"] - ref["var"]) / case["pv"][:, None]).max())
    assert np.all(np.abs(got["var"] - ref["var"]) <= G.RTOL * case["pv"][:, None])


def test_nan_is_picked_first(bo):
    case = grid_case(2)
    cands = grid_set(bo, case)
    free = np.flatnonzero(~case["excluded"])
    a, b = int(free[7]), int(free[-3])
    assert a not in case["ref"]["idx"] and b not in case["ref"]["idx"]
    base = case["base"].copy()
    base[a] = np.nan
    got = run(bo, case, cands, base=base)
    assert got["top_idx"][0] == a and np.isnan(got["top_val"][0])
    # a NaN in var: acq_1 is `base` bit for bit, so it enters with the first penalised array
    var0 = case["ref"]["var0"].copy()
    var0[1, b] = np.nan
    got = run(bo, case, cands, var0=var0)
    assert got["top_idx"][0] == case["ref"]["idx"][0]
    assert got["top_idx"][1] == b and np.isnan(got["top_val"][1]) and np.isnan(got["acq_last"][b])
    assert np.isnan(got["acq_last"]).sum() == 1


def test_float32_branch_constants(bo):
    """jitter 1e-3 and the floor 1e-6 are passed through: explicitly, and by float_type."""
    case = grid_case(2, jitter=1e-3, min_var=1e-6)
    assert_margins(case["ref"])
    cands = grid_set(bo, case)
    got = run(bo, case, cands)
    check_parity(case, got)
    assert got["var"].min() >= 1e-6
    by_type = run(bo, case, cands, jitter=None, min_variance=None, float_type=np.float32)
    for k in got:
        assert got[k].tobytes() == by_type[k].tobytes(), k
    default = run(bo, case, cands, jitter=None, min_variance=None)           # the f64 constants: another variance
    assert default["var"].tobytes() != got["var"].tobytes()
    # a floor that bites (above the variance left at the data and the picks, ~ jitter)
    hi = grid_case(2, jitter=1e-3, min_var=5e-3)
    got = run(bo, hi, cands)
    ref = G.gibbon_reference(hi["x"], hi["y"], hi["pts"], hi["pm"], hi["pv"], hi["ls"], 1e-3, 5e-3, 5, hi["excluded"],
                             hi["base"], picks=got["top_idx"])
    assert np.all(np.abs(got["var"] - ref["var"]) <= G.RTOL * hi["pv"][:, None])
    assert got["var"].min() == 5e-3 and (got["var"] == 5e-3).sum() >= 24


# 7. determinism and graph replay (raw ABI calls)
def raw_call(bo, case, ws=None):
    """(lib, desc, outputs, keepalive, workspace) of a grid call through the C ABI."""
    import torch
    from bayesopt_smart_amd import _lib
    from bayesopt_smart_amd.acquisition import ExclusionMask
    lib = _lib.load()
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")  # noqa: E731
    keep = dict(x=t(case["x"]), kinv=t(case["kinv"]), base=t(case["base"]), var=t(case["ref"]["var0"]))
    cands = grid_set(bo, case)
    keep["mask"] = ExclusionMask(cands, 0, cands.n, "cuda").update(TB.evaluated_of(case))
    n_obj, m, q = len(case["pv"]), cands.n, case["q"]
    out = dict(top_val=torch.zeros(q, dtype=torch.float64, device="cuda"),
               top_idx=torch.zeros(q, dtype=torch.int64, device="cuda"),
               var=torch.zeros((n_obj, m), dtype=torch.float64, device="cuda"),
               acq=torch.zeros(m, dtype=torch.float64, device="cuda"))
    d = _lib.GibbonDesc()
    d.n_obj, d.dim, d.n_train = n_obj, 2, case["x"].shape[0]
    d.x_train, d.kinv, d.ld_k = keep["x"].data_ptr(), keep["kinv"].data_ptr(), case["x"].shape[0]
    d.cand_kind, d.q, d.n_cand, d.cand_offset = _lib.CAND_GRID, q, m, 0
    for k in range(2):
        d.grid_lo[k], d.grid_shape[k] = GRID_LO[k], GRID_SHAPE[k]
    for o in range(n_obj):
        d.prior_var[o], d.length_scale[o] = case["pv"][o], case["ls"][o]
    d.jitter, d.min_variance = case["jitter"], case["min_var"]
    d.base, d.var, d.ld, d.mask = keep["base"].data_ptr(), keep["var"].data_ptr(), m, keep["mask"].ptr
    d.top_val, d.top_idx = out["top_val"].data_ptr(), out["top_idx"].data_ptr()
    d.var_out, d.acq_last = out["var"].data_ptr(), out["acq"].data_ptr()
    nbytes = lib.bo_select_batch_gibbon_workspace_size(ctypes.byref(d))
    assert nbytes > 0
    if ws is None:
        ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    return lib, d, out, keep, ws


def test_determinism_and_graph_replay(bo):
    import torch
    case = grid_case(5)
    lib, d, out, keep, ws = raw_call(bo, case)
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.bo_select_batch_gibbon(ctypes.byref(d), ws.data_ptr(), ws.numel(), stream) == 0
    direct = TB.snapshot(out)
    np.testing.assert_array_equal(out["top_idx"].cpu().numpy(), case["ref"]["idx"])
    # a second direct call, over a workspace of garbage: bit-identical
    ws.fill_(0xA5)
    for v in out.values():
        v.zero_()
    assert lib.bo_select_batch_gibbon(ctypes.byref(d), ws.data_ptr(), ws.numel(), stream) == 0
    assert TB.snapshot(out) == direct
    # captured on a side stream (there is no host step), replayed twice over a workspace of 0xFF bytes
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side, capture_error_mode="relaxed"):
            assert lib.bo_select_batch_gibbon(ctypes.byref(d), ws.data_ptr(), ws.numel(), side.cuda_stream) == 0
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        ws.fill_(0xFF)
        for v in out.values():
            v.zero_()
        g.replay()
        assert TB.snapshot(out) == direct


# 8. the loop: the fit is held at the given hyper-parameters (see test_gpu_bucb's loop)
LOOP_BOUNDS = [(-5, 28), (100, 131)]
LOOP_LS = np.array([6.0, 5.0, 7.0, 5.5, 6.5])
LOOP_PV = np.array([0.3, 0.5, 0.4, 0.35, 0.45])


def toy_function(x):
    """Five smooth objectives of a 2-D point."""
    a, b = (x[0] + 5.0) / 33.0, (x[1] - 100.0) / 31.0
    return np.array([-(a - 0.3) ** 2 - (b - 0.6) ** 2, np.sin(3.0 * a) + 0.5 * b, -(a - 0.8) ** 2 + 0.3 * np.cos(4.0 * b),
                     0.7 * a - (b - 0.2) ** 2, np.cos(2.0 * a + b)])


def loop_initial_points():
    rng = np.random.default_rng(25)
    pts = TB.grid_points(GRID_LO, GRID_SHAPE)
    return pts[rng.choice(pts.shape[0], 10, replace=False)]


def run_loop(bo, states=None, **kw):
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

        def select(self, *a, **k):
            idx = DeviceBackend.select(self, *a, **k)
            if states is not None:
                states.append(dict(x=a[0][0].clone(), y=a[0][1].clone(), kinv=a[0][2].clone(), idx=np.array(idx),
                                   var=self.bufs.variance_objectives.clone(), mu=self.bufs.mu_objectives.clone(),
                                   acq=self.bufs.acquisition_values.clone()))
            return idx

    opt = bo.BayesianOptimization(toy_function, LOOP_BOUNDS, n_objectives=5, n_iterations=2, batch_size=4,
                                  initial_points=loop_initial_points(), length_scales=LOOP_LS.copy(),
                                  prior_variance=LOOP_PV.copy(), betas=[2.0] * 5, acquisition="mes", mes_samples=4,
                                  ts_features=128, ts_seed=7, **kw)
    opt._backend = FixedFit(opt.candidates, 5, opt.total_samples, opt.device, ts_features=128, ts_seed=7,
                            mes_samples=4)
    opt._buffers = opt._backend.bufs
    opt.optimize()
    return opt


def test_loop_gibbon_is_the_public_pieces(bo):
    import torch
    from bayesopt_smart_amd import acquisition as A
    states = []
    opt = run_loop(bo, states, batch_strategy="gibbon")
    assert len(states) == 2
    xs = opt.x_vector
    assert len({tuple(r) for r in xs.tolist()}) == 18                   # 8 new points, all distinct
    pts = TB.grid_points(GRID_LO, GRID_SHAPE)
    cands = opt.candidates
    rng = np.random.default_rng(7)                                      # the backend's generator, replayed
    for s in states:
        n = s["x"].shape[0]
        draws = A.thompson_draws(rng, 5, 2, n, 4, 128)
        paths = A.sample_paths(s["x"], s["y"], s["kinv"], cands, opt.prior_mean, LOOP_PV, LOOP_LS, draws,
                               device="cuda")
        ystar = A.path_maxima(paths, opt.prior_mean, LOOP_PV)
        acq = A.max_value_entropy(s["mu"], s["var"], ystar)
        assert torch.equal(acq, s["acq"])                               # the callbacks see the plain array
        keep = (acq.clone(), s["var"].clone())
        idx = A.select_batch_gibbon(acq, s["var"], s["x"], s["kinv"], cands, LOOP_PV, LOOP_LS, s["x"].cpu().numpy(), 4)
        assert torch.equal(acq, keep[0]) and torch.equal(s["var"], keep[1]), "the inputs were modified"
        print("batch", s["idx"], "replay", idx)
        np.testing.assert_array_equal(s["idx"], idx)
        top = A.select_indices(acq, cands, s["x"].cpu().numpy(), 4)
        assert s["idx"][0] == top[0] and s["idx"].tolist() != top.tolist()
    np.testing.assert_array_equal(xs[10:14], pts[states[0]["idx"]])


def test_loop_top_is_unchanged(bo):
    a = run_loop(bo)
    b = run_loop(bo, batch_strategy="top")
    np.testing.assert_array_equal(a.x_vector, b.x_vector)
    np.testing.assert_array_equal(a.y_vector, b.y_vector)
    states = []
    run_loop(bo, states, batch_strategy="top")
    from bayesopt_smart_amd import acquisition as A
    for s in states:                                                    # "top": the masked top-q of the array
        np.testing.assert_array_equal(s["idx"], A.select_indices(s["acq"], a.candidates, s["x"].cpu().numpy(), 4))

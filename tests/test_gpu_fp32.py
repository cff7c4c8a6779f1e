"""BO_PREDICT_FP32 (BASELINE config C5: "fp32 with fp64 reference check"): the f32 matrix-core
variant of the fused predict + acquisition kernel against the f64 oracle.

Tolerances (written here; the rule of tests/test_gpu_c5_shards.py): in standardised units the f32
contraction leaves |d std_mu| <= EPS_MU and |d std_var| <= EPS_VAR; the UCB's square root
propagates |d sqrt(v)| <= min(sqrt(dv), dv / sqrt(v_ref)), so candidate i's acquisition bound is
    tol_i = sum_o EPS_MU + beta_o min(sqrt(EPS_VAR), EPS_VAR / sqrt(std_var_ref[o, i]))
-- ~1e-4 away from the data, ~1e-2 at a training point -- and the selection is judged tie-aware
on the CPU acquisition array with that per-candidate bound (round 3 allowed 0.19 max|acq| and
only asked each pick to lie within 2x that of the 16th best).
The counted f32 rounding bound of this kernel, at small shapes: tests/test_gpu_fp32_exact.py."""
import numpy as np
import pytest

from oracle import oracle_np as O
from fullref import cpu_full
from parity import check_topq

pytestmark = pytest.mark.gpu

EPS_MU = 1e-5           # |d std_mu| (6-D designs at ls 40: measured <= 2.6e-6 on C5's shards)
EPS_VAR = 1e-5          # |d std_var|
EPS_2D = 1e-4           # the 2-D grid design at ls 6 (cond(K) ~1e4): measured 5.9e-5 / 3.0e-5


def acq_bound(ref_var, pv, betas, eps_mu=EPS_MU, eps_var=EPS_VAR):
    """Per-candidate acquisition bound tol_i of the module docstring."""
    pv, betas = np.asarray(pv)[:, None], np.asarray(betas)[:, None]
    sv = np.maximum(np.asarray(ref_var) / pv, 1e-300)
    return np.sum(eps_mu + betas * np.minimum(np.sqrt(eps_var), eps_var / np.sqrt(sv)), axis=0)


@pytest.fixture(scope="module")
def bo():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import bayesopt_smart_amd as bo
    bo._lib.load()
    return bo


def test_mfma_f32_layout(bo):
    import torch
    rng = np.random.default_rng(0)
    a = rng.normal(size=(16, 4)).astype(np.float32)
    b = rng.normal(size=(4, 16)).astype(np.float32)
    ta, tb = torch.as_tensor(a, device="cuda"), torch.as_tensor(b, device="cuda")
    td = torch.empty((16, 16), dtype=torch.float32, device="cuda")
    bo._lib.check(bo._lib.load().bo_selftest_mfma_f32(ta.data_ptr(), tb.data_ptr(), td.data_ptr(), None),
                  "selftest")
    torch.cuda.synchronize()
    np.testing.assert_allclose(td.cpu().numpy(), a.astype(np.float64) @ b, rtol=1e-5, atol=1e-5)


def _problem(rng, n, dim, n_obj, cand, ls):
    x = cand[rng.choice(cand.shape[0], n, replace=False)].astype(np.float64)
    y = rng.normal(size=(n, n_obj)) * 40 + 7
    pm, pv = y.mean(0), y.var(0)
    lsv = np.full(n_obj, ls)
    betas = rng.uniform(0.5, 2.5, size=n_obj)
    km = np.zeros((n_obj, n, n))
    O.update_k(km, x, 0, n, pv, lsv)
    kinv = O.invert_k(n, km)
    return x, y, pm, pv, lsv, betas, kinv


@pytest.mark.parametrize("n,dim,n_obj,m,ls", [(300, 6, 3, 20000, 40.0), (2048, 6, 3, 65536, 40.0),
                                              (100, 2, 2, 0, 6.0)])
def test_fp32_vs_f64_oracle(bo, n, dim, n_obj, m, ls):
    import torch
    rng = np.random.default_rng(n)
    if m:
        from scipy.stats import qmc
        cand = qmc.Sobol(dim, scramble=False).random(m) * 300.0
        cands = bo.CandidateSet.explicit(cand)
    else:
        cands = bo.CandidateSet.grid([(0, 128), (0, 96)])
        cand = O.grid_points([(0, 128), (0, 96)]).astype(np.float64)
        m = cand.shape[0]
    x, y, pm, pv, lsv, betas, kinv = _problem(rng, n, dim, n_obj, cand, ls)
    res = bo.predict_acquire(x, y, kinv, cands, pm, pv, lsv, betas, outputs=("mu", "var", "acq"),
                             topq=16, mode="fp32")
    torch.cuda.synchronize()
    got = {k: res[k].cpu().numpy() for k in ("mu", "var", "acq", "top_idx")}
    # every candidate against the f64 CPU reference (oracle/cpu_ref.c)
    ref = cpu_full(("fp32", n, dim, m), x, y, cand, kinv, pm, pv, lsv, betas)
    dmu = np.abs(got["mu"] - ref["mu"]) / np.sqrt(pv)[:, None]
    dvar = np.abs(got["var"] - ref["var"]) / pv[:, None]
    print(f"fp32 N={n} d={dim}: max |d std_mu| {dmu.max():.3e}, max |d std_var| {dvar.max():.3e}")
    eps = EPS_2D if dim == 2 else EPS_MU
    assert dmu.max() <= eps, dmu.max()
    assert dvar.max() <= eps, dvar.max()
    tol = acq_bound(ref["var"], pv, betas, eps, eps)
    da = np.abs(got["acq"] - ref["acq"])
    bad = da > tol
    assert not bad.any(), (int(bad.sum()), da[bad][:5], tol[bad][:5])
    xs = {tuple(r) for r in x}
    excl = np.array([tuple(c) in xs for c in cand])
    check_topq(got["top_idx"], ref["acq"], excl, 16, tol=tol)


def test_float32_branch_loop_iteration_c5_shape(bo):
    """BASELINE C5's shape through the drop-in API in the reference's float32 branch
    (BayesianOptimization(float_type=np.float32): config.py:54-66 jitters and variance floor,
    COBYLA for the fit, numba_kernels.py:290-302; the predict on the f32 matrix cores): 2048
    initial points drawn from the 2^22-point Sobol set, one iteration of q = 16 over the whole set,
    the objectives toy_function_3d plus a ripple of period ~75 (the smooth quadratic alone drives
    the fitted length scales to ~260, where cond(K) ~1e15 makes any K^-1 -- LAPACK's, the device's,
    and certainly an f32 contraction -- meaningless; SURVEY.md §8c's parity regime).  The
    iteration's acquisition array is checked against the f64 CPU reference with the iteration's
    own fitted hyper-parameters and K^-1 (invert_k with the float32 jitter 1e-3) and the float32
    floor (1e-6), on a 2^17-candidate prefix, with the per-candidate bound."""
    import torch
    import bench
    from bayesopt_smart_amd.bayesian_optimization import BayesianOptimization
    from oracle import cpu_ref
    cfg = bench.CONFIGS["C5"]
    cs = bo.CandidateSet.sobol_set(cfg["dim"], cfg["m"], scale=300.0)
    rng = np.random.default_rng(11)
    x0 = cs.points(rng.choice(cfg["m"], size=cfg["n_train"], replace=False))

    def f3(p):
        p = np.asarray(p, dtype=np.float64)
        base = bench.toy_function_3d(p[None])[0]
        return base + 4000.0 * np.array([np.sin(p[0] / 12.0) * np.cos(p[3] / 12.0),
                                         np.sin(p[1] / 12.0) * np.cos(p[4] / 12.0),
                                         np.sin(p[2] / 12.0) * np.cos(p[5] / 12.0)])
    seen = []
    opt = BayesianOptimization(f3, [(0, 300)] * 6, n_objectives=3, n_iterations=1, batch_size=16,
                               initial_points=x0, input_space=cs, float_type=np.float32,
                               length_scales=np.full(3, 40.0), betas=np.full(3, 2.0),
                               callbacks=[lambda st: seen.append({"x_next": np.array(st["x_next"]),
                                                                  "t": dict(st["timings"])})])
    assert opt.x_vector.dtype == np.float32 and opt.y_vector.dtype == np.float32
    n = cfg["n_train"]
    pm = opt.prior_mean.astype(np.float64)
    opt.optimize()
    torch.cuda.synchronize()
    assert len(seen) == 1 and seen[0]["x_next"].shape == (16, 6)
    ls, pv = opt.length_scales.astype(np.float64), opt.prior_variance.astype(np.float64)
    betas = opt.betas.astype(np.float64)
    x = opt.x_vector[:n].astype(np.float64)
    y = opt.y_vector[:n].astype(np.float64)
    # the iteration's K^-1: the same device update_k + invert_k (float32 jitter) at the fitted values
    km = torch.zeros((3, n, n), dtype=torch.float64, device="cuda")
    xd = torch.tensor(x, device="cuda")
    bo.kernels.update_k(km, xd, 0, n, pv, ls)
    kinv = bo.kernels.invert_k(n, km, float_type=np.float32).cpu().numpy()
    conds = [np.linalg.cond(km[o].cpu().numpy() + 1e-3 * np.eye(n)) for o in range(3)]
    print(f"float32 C5-shape iteration: fitted ls {ls}, cond(K + 1e-3 I) {['%.1e' % c for c in conds]}, "
          f"timings {seen[0]['t']}")
    m = 1 << 17
    pts = cs.points(np.arange(m))
    ref = cpu_ref.predict_acquire(x, y, pts, kinv, pm, pv, ls, betas, ucb=True)
    var = np.maximum(ref["var"], 1e-6)                                        # MIN_VARIANCE f32
    acq_ref = np.sum((ref["mu"] - pm[:, None]) / np.sqrt(pv)[:, None]
                     + betas[:, None] * np.sqrt(np.abs(var / pv[:, None])), axis=0)
    got = opt.acquisition_values[:m]
    tol = acq_bound(var, pv, betas, *f32_model_eps(x, y, pts, kinv, pm, pv, ls))
    da = np.abs(got - acq_ref)
    print(f"max |d acq| {da.max():.3e} (bound at that candidate {tol[np.argmax(da)]:.3e}), "
          f"max |d acq| / bound {np.max(da / tol):.3f}")
    bad = da > tol
    assert not bad.any(), (int(bad.sum()), da[bad][:5], tol[bad][:5])


F32_MODEL_C = 16.0      # units of 2^-24 per term: k* (exp of an f32 argument), K^-1 and alpha cast to
                        # f32, the product, and the blocked f32 accumulation


def f32_model_eps(x, y, pts, kinv, pm, pv, ls):
    """Per-candidate first-order bound of the f32 contraction's error in standardised units
    (float32 rounding of k*, K^-1 and the products; no cancellation credit):
        |d std_mu|_oi  <= C u sum_j |k_ij| |alpha_oj| / sqrt(pv_o)
        |d std_var|_oi <= C u sum_jl |k_ij| |K^-1_o,jl| |k_il| / pv_o,   u = 2^-24,
    floored at EPS_MU / EPS_VAR.  At fitted length scales cond(K) reaches 1e5..1e6, where the
    variance's cancellation (pv - k K^-1 k) loses that many f32 ulps -- the f32 branch's own
    behaviour (the reference's float32 branch keeps K^-1 itself in float32).  Computed in f64 on
    the device (the checker, not the product: plain torch matmuls)."""
    import torch
    u = 2.0 ** -24
    xd = torch.tensor(x, device="cuda")
    eps_mu, eps_var = [], []
    for o in range(kinv.shape[0]):
        ki = torch.tensor(kinv[o], device="cuda")
        alpha = ki @ torch.tensor(y[:, o] - pm[o], device="cuda")
        aki = ki.abs()
        emu, evar = [], []
        for c0 in range(0, pts.shape[0], 1 << 14):
            p = torch.tensor(pts[c0:c0 + (1 << 14)], device="cuda")
            k = (pv[o] * torch.exp(-0.5 * torch.cdist(p, xd) ** 2 / ls[o] ** 2)).abs()
            emu.append((k @ alpha.abs()) / np.sqrt(pv[o]))
            evar.append(((k @ aki) * k).sum(1) / pv[o])
        eps_mu.append(np.maximum(EPS_MU, F32_MODEL_C * u * torch.cat(emu).cpu().numpy()))
        eps_var.append(np.maximum(EPS_VAR, F32_MODEL_C * u * torch.cat(evar).cpu().numpy()))
    return np.array(eps_mu), np.array(eps_var)

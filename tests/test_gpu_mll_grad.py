"""GPU tests of bo_compute_mll_grad (the MLL terms and their analytic gradients in log l), of the L-BFGS fit
built on it (optimize_hyperparams_mll, method="lbfgs") and of fit_method="lbfgs" through the loop.

The value is compute_mll's, bit for bit, kernel_matrix included.  The gradient is held to the long-double
reference of tests/mll_grad_ref.py by DESIGN section 5's 8 R rule: err / (u S) <= 8 R on every objective of every
case, S the first-order scale derived there and R the largest such ratio of the f64 numpy restatement
(np.linalg.inv + one Newton step) over the same cases, computed on the CPU in this process."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import exact_fit_ref as F
import mll_grad_ref as G
from bayesopt_smart_amd.config import HYPERPARAM_FTOL
from test_gpu_fit import _problem as _fit_problem
from test_gpu_fit_workspace import _Guarded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_DEVICE = {}


@pytest.fixture(scope="module")
def bo():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import bayesopt_smart_amd as bo
    bo._lib.load()
    return bo


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def _device(bo, key):
    """One 3-objective compute_mll_grad call per case, shared by the value and the gradient tests: (terms,
    gradients, kernel_matrix afterwards)."""
    import torch
    if key not in _DEVICE:
        p = F.mll_problem(key)
        n = p["n"]
        km = torch.zeros((3, n, n), dtype=torch.float64, device="cuda")
        val, grad = bo.kernels._mll_grad_call(torch.tensor(p["x"], device="cuda"), torch.tensor(p["y"], device="cuda"),
                                              km, p["pm"], p["pv"], p["ls"], n, p["jitter"])
        _DEVICE[key] = (val, grad, km.cpu().numpy())
    return _DEVICE[key]


# 1. the value
@pytest.mark.parametrize("key", G.VALUE_CASES, ids=lambda k: f"n{k[0]}")
def test_value_and_kernel_matrix_are_compute_mlls_bits(bo, key):
    import torch
    p = F.mll_problem(key)
    n = p["n"]
    val, _, km = _device(bo, key)
    km_ref = torch.zeros((3, n, n), dtype=torch.float64, device="cuda")
    ref = bo.kernels._mll_terms(torch.tensor(p["x"], device="cuda"), torch.tensor(p["y"], device="cuda"), km_ref,
                                p["pm"], p["pv"], p["ls"], n, [0, 1, 2], jitter=p["jitter"])
    want = np.array([ref[o] for o in range(3)])
    assert np.all(np.isfinite(want))
    assert _bits(val) == _bits(want), (val, want)
    assert km.tobytes() == km_ref.cpu().numpy().tobytes()


def test_public_entry_point_numpy_in(bo):
    """kernels.compute_mll_grad with numpy arrays: the device call's bits, kernel_matrix copied back, and the
    terms sum to compute_mll."""
    key = (33, 1e-8, "")
    p = F.mll_problem(key)
    km = np.zeros((3, 33, 33))
    val, grad = bo.kernels.compute_mll_grad(p["x"], p["y"], km, p["pm"], p["pv"], p["ls"], 33)
    dval, dgrad, dkm = _device(bo, key)
    assert isinstance(val, np.ndarray) and isinstance(grad, np.ndarray) and val.shape == grad.shape == (3,)
    assert _bits(val) == _bits(dval) and _bits(grad) == _bits(dgrad) and km.tobytes() == dkm.tobytes()
    tot = bo.kernels.compute_mll(p["x"], p["y"], np.zeros((3, 33, 33)), p["pm"], p["pv"], p["ls"], 33)
    assert tot == (val[0] + val[1]) + val[2]


CHILD = r"""
import json, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import bayesopt_smart_amd as bo
import exact_fit_ref as F
p = F.mll_problem((65, 1e-8, ""))
xd, yd = torch.tensor(p["x"], device="cuda"), torch.tensor(p["y"], device="cuda")
km = torch.zeros((3, 65, 65), dtype=torch.float64, device="cuda")
before = bo._lib.fit_path_counts()
val, grad = bo.kernels._mll_grad_call(xd, yd, km, p["pm"], p["pv"], p["ls"], 65, 1e-8)
after = bo._lib.fit_path_counts()
km_ref = torch.zeros_like(km)
ref = bo.kernels._mll_terms(xd, yd, km_ref, p["pm"], p["pv"], p["ls"], 65, [0, 1, 2], jitter=1e-8)
print("RESULT " + json.dumps(dict(val=[v.hex() for v in val], ref=[float(ref[o]).hex() for o in range(3)],
                                  grad=[float(g) for g in grad], km_equal=bool(torch.equal(km, km_ref)),
                                  moved={k: after[k] - before[k] for k in after})))
"""


def test_value_bits_on_the_launch_per_step_path(bo):
    """n = 65 in a child process under BO_FIT_PATH=launches: both factorisations of the call (the value's and
    the inverse's) ran launch per step, none persistent; the value is compute_mll's on that path, bit for bit,
    and the gradient meets the same rule as on the persistent path."""
    env = dict(os.environ, BO_FIT_PATH="launches")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    c = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("RESULT "))[7:])
    assert c["moved"] == {"persistent": 0, "launches": 2, "aborted": 0}, c["moved"]
    assert c["val"] == c["ref"] and c["km_equal"], c
    R = G.grad_R()
    for o, ref in enumerate(G.grad_case((65, 1e-8, ""))["grefs"]):
        assert G.grad_ratio(c["grad"][o], ref) <= G.TIGHT * R, (o, c["grad"][o], ref["g"])


# 2. the gradient
@pytest.mark.parametrize("key", G.GRAD_CASES, ids=lambda k: f"n{k[0]}-{k[1]:g}{k[2]}")
def test_gradient_against_the_long_double_reference(bo, key):
    import torch
    p, c = F.mll_problem(key), G.grad_case(key)
    n = p["n"]
    _, grad, _ = _device(bo, key)
    R = G.grad_R()
    for o in range(3):
        ref = c["grefs"][o]
        ratio = G.grad_ratio(grad[o], ref)
        print(f"{key} objective {o} (l = {p['ls'][o]:.4g}): g {grad[o]:.15g} (reference {ref['g']:.15g}), "
              f"err / (u S) {ratio:.3g} (restatement {G.grad_ratio(c['restated'][o], ref):.3g}, 8 R = {G.TIGHT * R:.4g})")
        assert np.isfinite(grad[o])
        assert ratio <= G.TIGHT * R, (key, o, ratio, R)
        if n == 1:
            assert grad[o] == 0.0
    # objective 1 alone, at its own length scale: the 3-objective call's bits for it
    km1 = torch.zeros((1, n, n), dtype=torch.float64, device="cuda")
    v1, g1 = bo.kernels._mll_grad_call(torch.tensor(p["x"], device="cuda"),
                                       torch.tensor(np.ascontiguousarray(p["y"][:, 1:2]), device="cuda"), km1,
                                       p["pm"][1:2], p["pv"][1:2], p["ls"][1:2], n, p["jitter"])
    val, _, km = _device(bo, key)
    assert _bits(g1) == _bits(grad[1:2]) and _bits(v1) == _bits(val[1:2])
    assert km1.cpu().numpy().tobytes() == km[1:2].tobytes()


# 3. determinism
def test_two_calls_give_the_same_bits(bo):
    import torch
    key = (257, 1e-8, "")
    p = F.mll_problem(key)
    val, grad, km = _device(bo, key)
    km2 = torch.zeros((3, 257, 257), dtype=torch.float64, device="cuda")
    val2, grad2 = bo.kernels._mll_grad_call(torch.tensor(p["x"], device="cuda"), torch.tensor(p["y"], device="cuda"),
                                            km2, p["pm"], p["pv"], p["ls"], 257, 1e-8)
    assert _bits(val) == _bits(val2) and _bits(grad) == _bits(grad2) and km.tobytes() == km2.cpu().numpy().tobytes()


# 4. the workspace
def test_workspace_of_exactly_the_reported_size(bo):
    """test_gpu_fit_workspace.py's method: the call in a workspace of exactly the reported size between two
    guard regions, the buffer filled with 0xA5; the guards stay, the outputs are the ordinary workspace's."""
    import torch
    lib = bo._lib.load()
    key = (257, 1e-8, "")
    p = F.mll_problem(key)
    n = 257
    nbytes = lib.bo_compute_mll_grad_workspace_size(3, n)
    assert nbytes > 0 and nbytes % 256 == 0
    assert nbytes >= max(lib.bo_compute_mll_workspace_size(3, n), lib.bo_invert_k_workspace_size(3, n)) + 2 * 3 * n * n * 8
    assert lib.bo_compute_mll_grad_workspace_size(9, n) == 0
    assert lib.bo_compute_mll_grad_workspace_size(0, n) == 0 and lib.bo_compute_mll_grad_workspace_size(3, 0) == 0
    g = _Guarded(nbytes)
    xd, yd = torch.tensor(p["x"], device="cuda"), torch.tensor(p["y"], device="cuda")
    km = torch.zeros((3, n, n), dtype=torch.float64, device="cuda")
    vec = lambda v: (C.c_double * len(v))(*[float(a) for a in v])  # noqa: E731
    val, grad = (C.c_double * 3)(), (C.c_double * 3)()
    stream = bo.device.stream_handle(bo.device.require_device())
    st = lib.bo_compute_mll_grad(val, grad, xd.data_ptr(), p["dim"], yd.data_ptr(), yd.stride(0),
                                 km.data_ptr(), n, 3, vec(p["pm"]), vec(p["pv"]), vec(p["ls"]), n, 1e-8, g.ptr,
                                 g.nbytes, stream)
    g.check()
    assert st == bo._lib.OK, st
    dval, dgrad, dkm = _device(bo, key)
    assert _bits(list(val)) == _bits(dval) and _bits(list(grad)) == _bits(dgrad)
    assert km.cpu().numpy().tobytes() == dkm.tobytes()
    # one byte short: refused, nothing written
    st = lib.bo_compute_mll_grad(val, grad, xd.data_ptr(), p["dim"], yd.data_ptr(), yd.stride(0), km.data_ptr(), n, 3,
                                 vec(p["pm"]), vec(p["pv"]), vec(p["ls"]), n, 1e-8, g.ptr, g.nbytes - 1, stream)
    assert st == bo._lib.ERR_WORKSPACE
    g.check()


# 5. the error status
def test_not_positive_definite_raises_linalgerror(bo):
    """Two identical training rows and jitter 0: the second pivot is 1 - 1 * 1 = 0 exactly.  compute_mll's
    terms raise LinAlgError for it, and so does the gradient call (the value's status, returned first)."""
    import torch
    p = F.mll_problem((33, 1e-8, ""))
    x = p["x"].copy()
    x[1] = x[0]
    xd, yd = torch.tensor(x, device="cuda"), torch.tensor(p["y"], device="cuda")
    km = torch.zeros((3, 33, 33), dtype=torch.float64, device="cuda")
    with pytest.raises(np.linalg.LinAlgError):
        bo.kernels._mll_terms(xd, yd, km, p["pm"], p["pv"], p["ls"], 33, [0, 1, 2], jitter=0.0)
    with pytest.raises(np.linalg.LinAlgError):
        bo.kernels._mll_grad_call(xd, yd, km, p["pm"], p["pv"], p["ls"], 33, 0.0)
    # and the library works afterwards
    val, grad = bo.kernels._mll_grad_call(torch.tensor(p["x"], device="cuda"), yd, km, p["pm"], p["pv"], p["ls"], 33, 1e-8)
    dval, dgrad, _ = _device(bo, (33, 1e-8, ""))
    assert _bits(val) == _bits(dval) and _bits(grad) == _bits(dgrad)


# 6. the fit
@pytest.mark.parametrize("n,dim,n_obj", [(48, 2, 2), (96, 2, 2), (300, 6, 3)])
def test_lbfgs_fit_reaches_powells_mll_in_a_quarter_of_the_evaluations(bo, n, dim, n_obj):
    """test_gpu_fit.py's problem family (seed n + 1), both methods from the same start.  The problems were
    checked on the CPU first: mll_grad_ref.numpy_value_grad under scipy's L-BFGS-B and under scipy's Powell with
    the same options meets both conditions below on each of them (13-14 evaluations against 202-282, the MLL
    within 0.001 of the margin HYPERPARAM_FTOL |mll|)."""
    import torch
    x, y, pm, pv, ls = _fit_problem(n, dim, n_obj, n + 1)
    xd, yd = torch.tensor(x, device="cuda"), torch.tensor(y, device="cuda")
    km_p = torch.zeros((n_obj, n, n), dtype=torch.float64, device="cuda")
    ls_p, pv_p = ls.copy(), pv.copy()
    powell = bo.kernels.optimize_hyperparams_mll(xd, yd, km_p, pm, pv_p, ls_p, n, method="powell")
    km = torch.zeros((n_obj, n, n), dtype=torch.float64, device="cuda")
    ls_l, pv_l = ls.copy(), pv.copy()
    res = bo.kernels.optimize_hyperparams_mll(xd, yd, km, pm, pv_l, ls_l, n, method="lbfgs")
    mll_l, mll_p = -res.fun, -powell.fun
    print(f"N {n}: lbfgs nfev {res.nfev} nit {res.nit} device calls {res.device_calls} mll {mll_l!r} ls {ls_l.tolist()} "
          f"| powell nfev {powell.nfev} device calls {powell.device_calls} mll {mll_p!r} ls {ls_p.tolist()} | "
          f"(mll_p - mll_l) / (ftol |mll_p|) = {(mll_p - mll_l) / (HYPERPARAM_FTOL * abs(mll_p)):.3g}; {res.message}")
    assert mll_l >= mll_p - HYPERPARAM_FTOL * abs(mll_p)
    assert res.nfev < powell.nfev / 4
    assert _bits(pv_l) == _bits(pv)                                 # prior_variance: bit-unchanged
    assert res.x.shape == (2 * n_obj,)
    assert _bits(res.x[:n_obj]) == _bits(ls_l) and _bits(res.x[n_obj:]) == _bits(pv)
    assert np.all(np.isfinite(ls_l)) and np.all(ls_l > 0) and not np.array_equal(ls_l, ls)
    assert res.jac.shape == (n_obj,) and res.device_calls == res.nfev and isinstance(res.message, str)
    km_ref = torch.zeros_like(km)
    bo.kernels.update_k(km_ref, xd, 0, n, pv_l, ls_l)
    assert torch.equal(km, km_ref)
    # the result's MLL is the device's at the result
    tot = bo.kernels.compute_mll(xd, yd, torch.zeros_like(km), pm, pv_l, ls_l, n)
    assert tot == mll_l
    # method=None is the Powell path
    ls_n, pv_n = ls.copy(), pv.copy()
    none = bo.kernels.optimize_hyperparams_mll(xd, yd, torch.zeros_like(km), pm, pv_n, ls_n, n)
    assert _bits(none.x) == _bits(powell.x) and none.nfev == powell.nfev


# 7. the loop
LOOP_BOUNDS = [(-5, 28), (100, 131)]                      # 33 x 31 = 1023 candidates
LOOP_INITIAL = np.array([[-5, 100], [27, 130], [10, 115], [0, 125], [20, 105], [14, 110]])


def _toy(x):
    return np.array([-((x[0] - 12) ** 2) + 100, -((x[1] - 118) ** 2) + 20], dtype=np.float64)


def _toy_constrained(x):
    return np.append(_toy(x), 12.0 ** 2 - (x[0] - 5) ** 2 - (x[1] - 110) ** 2)


def _run_loop(bo, fn=_toy, **kw):
    states = []
    np.random.seed(11)
    opt = bo.BayesianOptimization(fn, LOOP_BOUNDS, n_objectives=2, n_iterations=3, batch_size=3,
                                  initial_points=LOOP_INITIAL, length_scales=[8.0] * (3 if "n_constraints" in kw else 2),
                                  acquisition="ehvi", reference_point=[-2000.0, -2000.0],
                                  callbacks=[lambda s: states.append({"hyperparams": np.array(s["hyperparams"]),
                                                                      "x_next": np.array(s["x_next"])})], **kw)
    pv0 = np.array(opt.prior_variance)
    opt.optimize()
    return opt, states, pv0


def _check_picks(opt, states, n_out):
    assert len(states) == 3 and opt.x_vector.shape == (15, 2)
    for s in states:
        assert s["hyperparams"].shape == (2 * n_out,) and np.all(np.isfinite(s["hyperparams"]))
        assert s["x_next"].shape == (3, 2)
    pts = opt.x_vector[:15]
    assert len({tuple(p) for p in pts.tolist()}) == 15        # distinct, and none evaluated before
    assert np.all(np.isfinite(opt.y_vector[:15]))


def test_loop_with_the_lbfgs_fit(bo):
    opt, states, pv0 = _run_loop(bo, fit_method="lbfgs")
    _check_picks(opt, states, 2)
    for s in states:
        assert _bits(s["hyperparams"][2:]) == _bits(pv0)      # the L-BFGS fit leaves pv as given
        assert np.all(s["hyperparams"][:2] != 8.0)            # both length scales were fitted
    assert _bits(opt.prior_variance) == _bits(pv0)


def test_loop_powell_is_the_default(bo):
    a, _, _ = _run_loop(bo)
    b, _, _ = _run_loop(bo, fit_method="powell")
    assert a.x_vector.tobytes() == b.x_vector.tobytes() and a.y_vector.tobytes() == b.y_vector.tobytes()
    with pytest.raises(ValueError, match="unknown fit method 'bogus'"):
        _run_loop(bo, fn=lambda x: (_ for _ in ()).throw(AssertionError("the objective ran")), fit_method="bogus")


def test_loop_lbfgs_fits_the_constraint_outputs_too(bo):
    opt, states, pv0 = _run_loop(bo, fn=_toy_constrained, fit_method="lbfgs", n_constraints=1,
                                 constraint_bounds=[(0.0, np.inf)])
    _check_picks(opt, states, 3)
    assert opt.y_vector.shape[1] == 3
    for s in states:
        assert np.all(s["hyperparams"][:3] != 8.0) and _bits(s["hyperparams"][3:]) == _bits(pv0)

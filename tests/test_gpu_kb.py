"""Kriging-believer batches for the EHVI (bo_select_batch_kb, acquisition.select_batch_kb,
batch_strategy="kb") against the numpy reference of tests/kb_ref.py: the posterior variance of a GP
trained on X u {picks} from the inverse of the augmented Gram matrix, the textbook EHVI per box, the
front extended by the posterior means at the picks.

Tolerances are the project's own (tests/parity.py, bucb_ref.RTOL): var within 1e-5 pv, acq within
1e-5 max(1, |ref|).  Every case asserts cond(K + jitter I) < 1e6 (make_case does).  A different pick
at step t changes every later step, so the selection precondition is asserted ON THE REFERENCE
ALONE: the best-to-second gap of every acq_t exceeds 10 tol max(1, |val|) (the seeds are the bucb
tests', whose gaps hold here too); the device's indices must then equal the reference's exactly.

The device call gets mu / var / kinv computed by numpy (the call is tested in isolation); the loop
test runs the whole pipeline.  The cases and the device helpers are test_gpu_bucb.py's.
"""
import ctypes
import functools

import numpy as np
import pytest

import kb_ref as R
from test_gpu_bucb import (LOOP_BOUNDS, LOOP_LS, LOOP_PV, cand_set, grid_case, grid_points, loop_initial_points,
                           make_case, make_fixed_fit_backend, shard_case, sobol_case, toy_function)

pytestmark = pytest.mark.gpu

TOL = R.RTOL
GRID = ((-5, 100), (33, 31))


@pytest.fixture(scope="module")
def bo():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import bayesopt_smart_amd as bo
    return bo


# --------------------------------------------------------------------------- references (numpy only)
def ref_point_of(case):
    return case["y"].min(axis=0) - 0.5


def reference(case, q=None, ref_point=None, excluded=None, picks=None, mu=None):
    """kb_ref over the case's shard (the bucb case supplies the data, the state and the exclusion)."""
    sl = slice(case["offset"], case["offset"] + case["count"])
    excluded = case["excluded"] if excluded is None else excluded
    ref_point = ref_point_of(case) if ref_point is None else ref_point
    return R.kb_reference(case["x"], case["y"], case["pts"][sl], case["pm"], case["pv"], case["ls"], case["jitter"],
                          case["min_var"], q or case["q"], excluded[sl], R.pareto_front(case["y"]), ref_point,
                          picks=picks, mu=mu)


@functools.lru_cache(maxsize=None)
def grid_ref(n, seed, q=5):
    return reference(grid_case(n, seed), q)


@functools.lru_cache(maxsize=None)
def sobol_ref():
    return reference(sobol_case())


@functools.lru_cache(maxsize=None)
def shard_ref():
    return reference(shard_case())


def assert_gaps(ref):
    """The selection precondition, on the reference alone."""
    print("gaps", ref["gaps"], "values", ref["val"])
    for t, (p, v, g) in enumerate(zip(ref["idx"], ref["val"], ref["gaps"])):
        if p >= 0:
            assert g > 10 * TOL * max(1.0, abs(v)), (t, g, v)


def sum_edges(case, ref, ref_point=None):
    """Per pick: the table form's S = sum_k E_k of the boxes that pick's scan walks."""
    import ehvi_ref as E
    from bayesopt_smart_amd.acquisition import hypervolume_boxes
    ref_point = ref_point_of(case) if ref_point is None else ref_point
    front = R.pareto_front(case["y"])
    out = []
    for t in range(len(ref["idx"])):
        cur = np.concatenate([front, ref["believed"][:t]])
        out.append(sum(E.edge_counts(hypervolume_boxes(cur, ref_point), len(ref_point))))
    return out


# --------------------------------------------------------------------------- device side
def run(bo, case, ref, cands, q=None, ref_point=None, excluded=None, **kw):
    import torch
    from bayesopt_smart_amd.acquisition import select_batch_kb
    mu = torch.as_tensor(np.ascontiguousarray(ref["mu"]), device="cuda")
    var = torch.as_tensor(np.ascontiguousarray(ref["var0"]), device="cuda")
    keep = (mu.clone(), var.clone())
    excluded = case["excluded"] if excluded is None else excluded
    kw.setdefault("jitter", case["jitter"])
    kw.setdefault("min_variance", case["min_var"])
    res = select_batch_kb(mu, var, case["x"], case["kinv"], cands, case["pv"], case["ls"], case["y"],
                          case["y"].shape[0], ref_point_of(case) if ref_point is None else ref_point,
                          case["pts"][excluded], q or len(ref["idx"]), offset=case["offset"], count=case["count"],
                          return_details=True, **kw)
    out = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}
    same = lambda a, b: a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()  # noqa: E731  (NaN-proof)
    assert same(mu, keep[0]) and same(var, keep[1]), "the inputs were modified"
    return out


def close(got, want, scale=None):
    """|got - want| <= tol max(1, |want|) (or tol scale); NaN exactly where the reference has NaN."""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    bound = TOL * (np.maximum(1.0, np.abs(want)) if scale is None else scale)
    return bool(np.all((np.abs(got - want) <= bound)[~nan]))


def check_parity(case, got, ref):
    want = np.where(ref["idx"] >= 0, ref["idx"] + case["offset"], -1)
    print("idx", got["top_idx"], "ref", want, "min gap", ref["gaps"].min(),
          "max |dvar|/pv", (np.abs(got["var"] - ref["var"]) / case["pv"][:, None]).max(),
          "max |dacq_first|", np.nanmax(np.abs(got["acq_first"] - ref["acq_first"])),
          "max |dacq_last|", np.nanmax(np.abs(got["acq_last"] - ref["acq_last"])), "boxes", got["n_boxes_max"])
    np.testing.assert_array_equal(got["top_idx"], want)
    ok = ref["idx"] >= 0
    assert close(got["top_val"][ok], ref["val"][ok])
    assert np.all(np.isneginf(got["top_val"][~ok]))
    assert close(got["var"], ref["var"], case["pv"][:, None] * np.ones_like(ref["var"]))
    assert close(got["acq_first"], ref["acq_first"])
    assert close(got["acq_last"], ref["acq_last"])
    # a believed vector is a copy of the mean at the pick (NaN rows where no candidate was left)
    assert got["believed"].tobytes() == np.ascontiguousarray(ref["believed"]).tobytes()
    assert got["n_boxes_max"] == ref["n_boxes"].max()


# 1. parity on a grid with a ragged last workgroup and wave: 33 x 31 = 1023 candidates
@pytest.mark.parametrize("n,seed", [(24, 1), (37, 2)])
def test_parity_grid(bo, n, seed):
    case, ref = grid_case(n, seed), grid_ref(n, seed)
    assert_gaps(ref)
    got = run(bo, case, ref, cand_set(bo, case, "grid", *GRID))
    check_parity(case, got, ref)
    assert len(set(got["top_idx"])) == 5 and not case["excluded"][got["top_idx"]].any()


# 2. consistency with the existing scan, bit for bit
def test_consistent_with_the_ehvi_scan(bo):
    from bayesopt_smart_amd.acquisition import _front_of, expected_hypervolume_improvement
    case, ref = grid_case(24, 1), grid_ref(24, 1)
    cands = cand_set(bo, case, "grid", *GRID)
    q5 = run(bo, case, ref, cands, q=5)
    q4 = run(bo, case, ref, cands, q=4)
    rp = ref_point_of(case)
    front = _front_of(case["y"], case["y"].shape[0], rp)
    first = expected_hypervolume_improvement(ref["mu"], ref["var0"], front, rp)
    assert q5["acq_first"].tobytes() == first.tobytes() == q4["acq_first"].tobytes()
    np.testing.assert_array_equal(q4["top_idx"], q5["top_idx"][:4])
    assert q4["believed"].tobytes() == q5["believed"][:4].tobytes()
    last = expected_hypervolume_improvement(ref["mu"], np.ascontiguousarray(q4["var"]),
                                            np.concatenate([front, q4["believed"]]), rp)
    assert q5["acq_last"].tobytes() == last.tobytes()


# 3. q = 1 is today's selection
def test_q1_is_the_ehvi_top1(bo):
    import torch
    from bayesopt_smart_amd.acquisition import ehvi_select_indices
    case, ref = grid_case(24, 1), grid_ref(24, 1)
    cands = cand_set(bo, case, "grid", *GRID)
    got = run(bo, case, ref, cands, q=1)
    acq = torch.empty(cands.n, dtype=torch.float64, device="cuda")
    top1 = ehvi_select_indices(acq, torch.as_tensor(ref["mu"], device="cuda"),
                               torch.as_tensor(ref["var0"], device="cuda"), case["y"], case["y"].shape[0],
                               ref_point_of(case), cands, case["pts"][case["excluded"]], 1)
    assert got["top_idx"].tolist() == top1.tolist() == [ref["idx"][0]]
    assert got["acq_first"].tobytes() == got["acq_last"].tobytes() == acq.cpu().numpy().tobytes()
    # var_out is the variance after that one pick, not the input variance
    one = reference(case, q=1)
    assert close(got["var"], one["var"], case["pv"][:, None] * np.ones_like(one["var"]))
    assert (got["var"] < ref["var0"] - 1e-3).any()


# 4. the forms agree: same picks, same bits; "table" runs with the edge count changing between picks
def test_forms_agree(bo):
    import ehvi_ref as E
    for case, ref, cands in [(grid_case(24, 1), grid_ref(24, 1), None), (grid_case(37, 2), grid_ref(37, 2), None),
                             (sobol_case(), sobol_ref(), "f64")]:
        cs = cand_set(bo, case, cands) if cands else cand_set(bo, case, "grid", *GRID)
        s = sum_edges(case, ref)
        print("sum_edges per pick", s)
        assert len(set(s)) > 1 and all(E.table_threads(v) == 256 for v in s)
        if len(case["pv"]) == 2:
            assert max(s) <= 40
        auto = run(bo, case, ref, cs)
        for form in ("direct", "table"):
            got = run(bo, case, ref, cs, form=form)
            np.testing.assert_array_equal(got["top_idx"], auto["top_idx"])
            assert got["acq_last"].tobytes() == auto["acq_last"].tobytes()
            assert got["acq_first"].tobytes() == auto["acq_first"].tobytes()
            assert got["var"].tobytes() == auto["var"].tobytes()


# 5. the candidate kinds agree: three objectives in 6-D, and the grid case
def test_kinds_agree_sobol_f64_6d(bo):
    case, ref = sobol_case(), sobol_ref()
    assert_gaps(ref)
    s = run(bo, case, ref, cand_set(bo, case, "sobol"))
    f = run(bo, case, ref, cand_set(bo, case, "f64"))
    np.testing.assert_array_equal(s["top_idx"], f["top_idx"])
    check_parity(case, s, ref)
    check_parity(case, f, ref)


def test_kinds_agree_grid_i64_f64(bo):
    case, ref = grid_case(24, 1), grid_ref(24, 1)
    g = run(bo, case, ref, cand_set(bo, case, "grid", *GRID))
    i = run(bo, case, ref, cand_set(bo, case, "i64"))
    f = run(bo, case, ref, cand_set(bo, case, "f64"))
    np.testing.assert_array_equal(g["top_idx"], i["top_idx"])
    np.testing.assert_array_equal(g["top_idx"], f["top_idx"])
    assert i["var"].tobytes() == f["var"].tobytes()
    check_parity(case, f, ref)


# 6. a shard: cand_offset 512, 400 of 1024 candidates
@pytest.mark.parametrize("kind", ["grid", "f64"])
def test_shard(bo, kind):
    case, ref = shard_case(), shard_ref()
    assert_gaps(ref)
    got = run(bo, case, ref, cand_set(bo, case, kind, (0, 0), (32, 32)))
    assert np.all((got["top_idx"] >= 512) & (got["top_idx"] < 912))
    check_parity(case, got, ref)


# 7. mask and exhaustion
def test_masked_argmax_is_never_returned(bo):
    from bayesopt_smart_amd.acquisition import ExclusionMask
    case = grid_case(24, 1)
    top = grid_ref(24, 1)["idx"][0]
    excluded = case["excluded"].copy()
    excluded[top] = True
    ref = reference(case, excluded=excluded)
    assert_gaps(ref)
    cands = cand_set(bo, case, "grid", *GRID)
    mask = ExclusionMask(cands, 0, cands.n, "cuda").update(case["pts"][excluded])
    before = mask.bits.cpu().numpy().tobytes()
    got = run(bo, case, ref, cands, excluded=excluded, mask=mask)
    assert top not in got["top_idx"] and len(set(got["top_idx"])) == 5
    check_parity(case, got, ref)
    assert mask.bits.cpu().numpy().tobytes() == before, "the caller's mask was modified"


def test_fewer_candidates_than_q(bo):
    case = grid_case(24, 1)
    excluded = np.ones(case["pts"].shape[0], dtype=bool)
    excluded[[40, 500, 1022]] = False                    # 1022: the last candidate of the ragged wave
    ref = reference(case, excluded=excluded)
    assert_gaps(ref)
    got = run(bo, case, ref, cand_set(bo, case, "grid", *GRID), excluded=excluded)
    assert sorted(got["top_idx"][:3]) == [40, 500, 1022] and got["top_idx"][3:].tolist() == [-1, -1]
    assert np.isnan(got["believed"][3:]).all()
    check_parity(case, got, ref)


# 8. / 12. raw ABI calls
def raw_call(bo, case, ref, q=5, box_capacity=256, ws=None, fill=0):
    """(lib, desc, outputs, keepalive, workspace) of a grid call through the C ABI; the workspace and
    the host staging start as `fill` bytes."""
    import torch
    from bayesopt_smart_amd import _lib
    from bayesopt_smart_amd.acquisition import ExclusionMask
    lib = _lib.load()
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")  # noqa: E731
    keep = dict(x=t(case["x"]), kinv=t(case["kinv"]), mu=t(ref["mu"]), var=t(ref["var0"]),
                front=np.ascontiguousarray(R.pareto_front(case["y"])), met=ctypes.c_int64(-1))
    cands = cand_set(bo, case, "grid", *GRID)
    keep["mask"] = ExclusionMask(cands, 0, cands.n, "cuda").update(case["pts"][case["excluded"]])
    n_obj, m = len(case["pv"]), cands.n
    z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device="cuda")  # noqa: E731
    out = dict(top_val=z(q), top_idx=z(q, dtype=torch.int64), believed=z(q, n_obj), var=z(n_obj, m),
               acq_first=z(m), acq_last=z(m))
    d = _lib.KbDesc()
    d.n_obj, d.dim, d.n_train = n_obj, 2, case["x"].shape[0]
    d.x_train, d.kinv, d.ld_k = keep["x"].data_ptr(), keep["kinv"].data_ptr(), case["x"].shape[0]
    d.cand_kind, d.q, d.n_cand, d.cand_offset = _lib.CAND_GRID, q, m, 0
    rp = ref_point_of(case)
    for k in range(2):
        d.grid_lo[k], d.grid_shape[k] = GRID[0][k], GRID[1][k]
    for o in range(n_obj):
        d.prior_var[o], d.length_scale[o], d.ref_point[o] = case["pv"][o], case["ls"][o], rp[o]
    d.jitter, d.min_variance = case["jitter"], case["min_var"]
    d.mu, d.var, d.ld, d.mask = keep["mu"].data_ptr(), keep["var"].data_ptr(), m, keep["mask"].ptr
    d.front, d.n_front = keep["front"].ctypes.data, keep["front"].shape[0]
    d.form, d.box_capacity = 0, box_capacity
    d.top_val, d.top_idx, d.believed = out["top_val"].data_ptr(), out["top_idx"].data_ptr(), out["believed"].data_ptr()
    d.var_out, d.acq_first, d.acq_last = out["var"].data_ptr(), out["acq_first"].data_ptr(), out["acq_last"].data_ptr()
    d.n_boxes_max = ctypes.pointer(keep["met"])
    nbytes = lib.bo_select_batch_kb_workspace_size(ctypes.byref(d))
    hbytes = lib.bo_select_batch_kb_host_workspace_size(ctypes.byref(d))
    assert nbytes > 0 and hbytes > 0
    if ws is None:
        ws = torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")
    keep["host"] = torch.full((hbytes,), fill, dtype=torch.uint8).pin_memory()
    d.host_ws, d.host_ws_bytes = keep["host"].data_ptr(), hbytes
    return lib, d, out, keep, ws


def snapshot(out):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().tobytes() for k, v in out.items()}


def test_box_capacity_too_small(bo):
    import torch
    from bayesopt_smart_amd import _lib
    case, ref = grid_case(24, 1), grid_ref(24, 1)
    nb = ref["n_boxes"]
    print("boxes per pick", nb)
    assert nb.max() > nb[0] > 2                           # the box count grows after the first pick
    stream = torch.cuda.current_stream().cuda_stream
    for cap in (2, int(nb[0])):                           # refused at once; refused at a later pick
        lib, d, out, keep, ws = raw_call(bo, case, ref, box_capacity=cap)
        assert lib.bo_select_batch_kb(ctypes.byref(d), ws.data_ptr(), ws.numel(), stream) == _lib.ERR_WORKSPACE
        torch.cuda.synchronize()
        assert keep["met"].value > cap
    roomy = run(bo, case, ref, cand_set(bo, case, "grid", *GRID))
    tight = run(bo, case, ref, cand_set(bo, case, "grid", *GRID), box_capacity=int(nb[0]))
    for k in ("top_idx", "top_val", "var", "acq_last", "believed"):
        assert tight[k].tobytes() == roomy[k].tobytes(), k
    assert tight["n_boxes_max"] == roomy["n_boxes_max"] == nb.max()


def test_abi_status_codes(bo):
    from bayesopt_smart_amd import _lib
    lib, d, out, keep, ws = raw_call(bo, grid_case(24, 1), grid_ref(24, 1))
    assert lib.bo_select_batch_kb(ctypes.byref(d), ws.data_ptr(), ws.numel() - 256, None) == _lib.ERR_WORKSPACE
    assert lib.bo_select_batch_kb(ctypes.byref(d), None, 0, None) == _lib.ERR_WORKSPACE
    d.host_ws_bytes -= 256
    assert lib.bo_select_batch_kb(ctypes.byref(d), ws.data_ptr(), ws.numel(), None) == _lib.ERR_WORKSPACE
    d.host_ws_bytes += 256
    d.ld = d.n_cand - 1
    assert lib.bo_select_batch_kb(ctypes.byref(d), ws.data_ptr(), ws.numel(), None) == _lib.ERR_ARG
    d.ld = d.n_cand
    d.var_out = d.var                                     # the inputs stay as they are
    assert lib.bo_select_batch_kb(ctypes.byref(d), ws.data_ptr(), ws.numel(), None) == _lib.ERR_ARG


# 9. believed vectors the boxes ignore: the reference point above the posterior mean of objective 0
def test_believed_vectors_the_boxes_ignore(bo):
    case = grid_case(24, 1)
    rp = ref_point_of(case)
    rp[0] = max(grid_ref(24, 1)["mu"][0].max(), case["y"][:, 0].max()) + 0.05
    ref = reference(case, ref_point=rp)
    assert_gaps(ref)
    assert np.all(ref["n_boxes"] == 1)                    # neither the front nor a believed vector bounds a box
    got = run(bo, case, ref, cand_set(bo, case, "grid", *GRID), ref_point=rp)
    check_parity(case, got, ref)
    assert got["n_boxes_max"] == 1


# 10. a NaN in mu at one unmasked candidate: it is pick 1, and the batch goes on
def test_nan_mean_is_picked_first(bo):
    case = grid_case(24, 1)
    j = 777
    assert not case["excluded"][j]
    mu = grid_ref(24, 1)["mu"].copy()
    mu[1, j] = np.nan
    ref = reference(case, mu=mu)
    assert ref["idx"][0] == j
    assert_gaps(ref)
    got = run(bo, case, ref, cand_set(bo, case, "grid", *GRID))
    rest = got["top_idx"][1:]
    assert got["top_idx"][0] == j and np.isnan(got["top_val"][0])
    assert np.isfinite(got["top_val"][1:]).all() and len(set(got["top_idx"])) == 5 and rest.min() >= 0
    assert not case["excluded"][rest].any()
    np.testing.assert_array_equal(got["top_idx"], ref["idx"])
    assert close(got["var"], ref["var"], case["pv"][:, None] * np.ones_like(ref["var"]))
    assert close(got["acq_last"], ref["acq_last"])


# 11. the float32 branch's constants: jitter 1e-3, floor 1e-6, taken from float_type
def test_float32_branch_constants(bo):
    # (37, 2): with these constants grid case (24, 1) has a reference gap of 4.9e-5 at pick 3, below the rule
    case = grid_case(37, 2, jitter=1e-3, min_var=1e-6)
    ref = reference(case)
    assert_gaps(ref)
    got = run(bo, case, ref, cand_set(bo, case, "grid", *GRID), float_type=np.float32, jitter=None,
              min_variance=None)
    check_parity(case, got, ref)
    assert got["var"].min() >= 1e-6


# 12. determinism; a workspace and a staging block of 0xFF bytes; a capturing stream is refused
def test_determinism_and_capture(bo):
    import torch
    from bayesopt_smart_amd import _lib
    case, ref = grid_case(24, 1), grid_ref(24, 1)
    lib, d, out, keep, ws = raw_call(bo, case, ref)
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.bo_select_batch_kb(ctypes.byref(d), ws.data_ptr(), ws.numel(), stream) == 0
    first = snapshot(out)
    np.testing.assert_array_equal(out["top_idx"].cpu().numpy(), ref["idx"])
    assert keep["met"].value == ref["n_boxes"].max()
    for v in out.values():
        v.zero_()
    assert lib.bo_select_batch_kb(ctypes.byref(d), ws.data_ptr(), ws.numel(), stream) == 0
    assert snapshot(out) == first
    lib, d2, out2, keep2, ws2 = raw_call(bo, case, ref, fill=0xFF)
    assert lib.bo_select_batch_kb(ctypes.byref(d2), ws2.data_ptr(), ws2.numel(), stream) == 0
    assert snapshot(out2) == first
    # the host waits inside the call, so it cannot be captured: refused before anything is launched
    for v in out.values():
        v.zero_()
    zeros = snapshot(out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side, capture_error_mode="relaxed"):
            st = lib.bo_select_batch_kb(ctypes.byref(d), ws.data_ptr(), ws.numel(), side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    assert st == _lib.ERR_UNSUPPORTED
    assert snapshot(out) == zeros
    assert lib.bo_select_batch_kb(ctypes.byref(d), ws.data_ptr(), ws.numel(), stream) == 0   # and works afterwards
    assert snapshot(out) == first


# 13. the loop, with test_gpu_bucb.py's toy function and fixed-fit backend
LOOP_REF_POINT = np.array([-1200.0, -1300.0])            # below every value of the toy function on the grid


def run_loop(bo, states=None, acqs=None, **kw):
    cb = None if acqs is None else [lambda state: acqs.append(np.array(state["acquisition_values"]))]
    opt = bo.BayesianOptimization(toy_function, LOOP_BOUNDS, n_objectives=2, n_iterations=2, batch_size=3,
                                  initial_points=loop_initial_points(), length_scales=LOOP_LS.copy(),
                                  prior_variance=LOOP_PV.copy(), betas=[2.0, 2.0], acquisition="ehvi",
                                  reference_point=LOOP_REF_POINT, callbacks=cb, **kw)
    opt._backend = make_fixed_fit_backend(opt, [] if states is None else states)
    opt._buffers = opt._backend.bufs
    opt.optimize()
    return opt


def loop_reference(x, y, pm):
    pts = grid_points((118, 118), (64, 64))
    excluded = (pts[:, None, :] == x[None, :, :]).all(-1).any(-1)
    _, cond = R.B.fitted_state(x, y, pm, LOOP_PV, LOOP_LS, 1e-6)
    assert cond.max() < 1e6, cond
    return R.kb_reference(x, y, pts, pm, LOOP_PV, LOOP_LS, 1e-6, 1e-10, 3, excluded, R.pareto_front(y),
                          LOOP_REF_POINT)


def test_loop_kb_matches_reference(bo):
    states, acqs = [], []
    opt = run_loop(bo, states, acqs, batch_strategy="kb")
    assert len(states) == 2 and len(acqs) == 2
    pts = grid_points((118, 118), (64, 64))
    for (x, y, idx), acq in zip(states, acqs):
        ref = loop_reference(x, y, opt.prior_mean)
        assert_gaps(ref)
        print("batch", idx, "ref", ref["idx"], "min gap", ref["gaps"].min())
        np.testing.assert_array_equal(idx, ref["idx"])
        # the callbacks see the EHVI array "top" would show: the first pick's acquisition.  The
        # mean and variance come from the device predict here: parity.py's rule on the inputs,
        # carried through the EHVI's derivatives (|d psi / d mu| <= 1, |d psi / d sigma| <= 0.4) -- checked
        # against the scale of the array, its largest value.
        assert np.all(np.abs(acq - ref["acq_first"]) <= TOL * np.maximum(1.0, np.abs(ref["acq_first"]).max()))
    np.testing.assert_array_equal(opt.x_vector[10:13], pts[states[0][2]])


def test_loop_top_is_untouched(bo):
    a = run_loop(bo)
    b = run_loop(bo, batch_strategy="top")
    np.testing.assert_array_equal(a.x_vector, b.x_vector)
    np.testing.assert_array_equal(a.y_vector, b.y_vector)

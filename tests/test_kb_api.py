"""The Kriging-believer batch for the EHVI without a GPU: the descriptor's layout, the workspace-size
queries' argument checks, the option's validation (no kernel is launched) and what the numpy
reference of tests/kb_ref.py does to a batch."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kb_desc_layout_matches_header():
    """ctypes mirror of bo_kb_desc has the C layout (checked against offsetof via a tiny C program
    compiled with gcc)."""
    import subprocess
    import tempfile
    from bayesopt_smart_amd import _lib
    fields = [f for f, _ in _lib.KbDesc._fields_]
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"bo_amd.h\"\nint main(){\n"
    prog += 'printf("%zu\\n", sizeof(bo_kb_desc));\n'
    for f in fields:
        prog += f'printf("%zu\\n", offsetof(bo_kb_desc, {f}));\n'
    prog += "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        vals = [int(v) for v in subprocess.check_output([exe]).split()]
    assert vals[0] == ctypes.sizeof(_lib.KbDesc)
    for f, off in zip(fields, vals[1:]):
        assert getattr(_lib.KbDesc, f).offset == off, f


def _desc():
    from bayesopt_smart_amd import _lib
    d = _lib.KbDesc()
    d.n_obj, d.dim, d.n_train, d.ld_k = 2, 2, 512, 512
    d.cand_kind, d.q, d.n_cand, d.ld = _lib.CAND_GRID, 3, 1 << 20, 1 << 20
    d.grid_shape[0] = d.grid_shape[1] = 1024
    for o in range(2):
        d.prior_var[o], d.length_scale[o], d.ref_point[o] = 1.0, 30.0, -1.0
    d.jitter, d.min_variance = 1e-6, 1e-10
    d.n_front, d.form, d.box_capacity = 16, 0, 64
    return d


def test_workspace_size_queries():
    from bayesopt_smart_amd import _lib
    lib = _lib.load()
    size = lambda d: lib.bo_select_batch_kb_workspace_size(ctypes.byref(d))  # noqa: E731
    host = lambda d: lib.bo_select_batch_kb_host_workspace_size(ctypes.byref(d))  # noqa: E731
    d = _desc()
    base, hbase = size(d), host(d)
    # without var_out the running variance lives in the workspace; no further candidate-sized array
    # but the per-workgroup bests (one entry per 64 candidates)
    assert 2 * (1 << 20) * 8 <= base < 2 * 2 * (1 << 20) * 8
    # host: the front with room for q believed rows, and one packed block of boxes, edges, indices
    assert (16 + 3) * 2 * 8 + 64 * 4 * 12 <= hbase < 16384
    d.var_out = 4096                                     # any non-NULL pointer: sizes only
    assert 0 < size(d) < base - 2 * (1 << 20) * 8 + 4096
    d = _desc()
    d.box_capacity = 128                                 # the box buffers grow with the capacity
    assert size(d) >= base + 64 * 4 * 12 and host(d) >= hbase + 64 * 4 * 12
    assert lib.bo_select_batch_kb_workspace_size(None) == 0
    assert lib.bo_select_batch_kb_host_workspace_size(None) == 0
    # what bo_select_batch_bucb's query rejects, and the front's and the scan's own fields
    for field, bad in [("q", 0), ("q", 49), ("n_obj", 9), ("n_obj", 0), ("dim", 9), ("n_train", 0),
                       ("ld_k", 511), ("n_cand", 0), ("ld", (1 << 20) - 1), ("cand_kind", 4),
                       ("cand_offset", 1), ("jitter", float("nan")), ("min_variance", -1.0),
                       ("n_obj", 5), ("form", 3), ("form", -1), ("box_capacity", 0), ("n_front", -1)]:
        d = _desc()
        setattr(d, field, bad)
        assert size(d) == 0 and host(d) == 0, (field, bad)
    for bad in (float("nan"), float("inf")):
        d = _desc()
        d.ref_point[1] = bad
        assert size(d) == 0 and host(d) == 0
    d = _desc()
    d.prior_var[1] = 0.0
    assert size(d) == 0
    d = _desc()
    d.length_scale[0] = float("nan")
    assert size(d) == 0


def test_call_checks_arguments_before_the_device():
    from bayesopt_smart_amd import _lib
    lib = _lib.load()
    d = _desc()
    d.q = 49
    assert lib.bo_select_batch_kb(ctypes.byref(d), None, 0, None) == _lib.ERR_ARG
    assert lib.bo_select_batch_kb(ctypes.byref(_desc()), None, 0, None) == _lib.ERR_ARG   # NULL arrays
    d = _desc()
    d.n_obj = 5
    assert lib.bo_select_batch_kb(ctypes.byref(d), None, 0, None) == _lib.ERR_ARG


def test_batch_strategy_validation(monkeypatch):
    from bayesopt_smart_amd import _lib, acquisition, distributed
    from bayesopt_smart_amd.bayesian_optimization import _check_batch_strategy, _check_limits
    assert acquisition.BATCH_STRATEGIES == ("top", "bucb", "ts")          # the pinned tuple is unchanged
    assert acquisition.ALL_BATCH_STRATEGIES == ("top", "bucb", "ts", "kb")
    _check_batch_strategy("kb", "ehvi", _lib.MAX_TOPQ)
    _check_limits(2, 2, 64, 3, "ehvi", "kb")
    for acq in ("sum_ucb", "hvi"):
        with pytest.raises(ValueError, match="ehvi"):
            _check_batch_strategy("kb", acq, 3)
    with pytest.raises(ValueError, match="batch_size <= 48"):
        _check_batch_strategy("kb", "ehvi", _lib.MAX_TOPQ + 1)
    with pytest.raises(ValueError, match="4 objectives"):
        _check_limits(5, 2, 64, 3, "ehvi", "kb")
    with pytest.raises(ValueError, match=r"unknown batch_strategy.*'top', 'bucb' or 'ts', or 'kb' with "
                                         r"acquisition='ehvi'\)"):
        _check_batch_strategy("believer", "ehvi", 3)
    monkeypatch.setattr(distributed, "collectives_on", lambda group=None: True)
    with pytest.raises(ValueError, match="one rank"):
        _check_batch_strategy("kb", "ehvi", 3)


def test_select_batch_kb_rejects_bad_arguments():
    from bayesopt_smart_amd import _lib
    from bayesopt_smart_amd.acquisition import select_batch_kb
    for q in (0, _lib.MAX_TOPQ + 1):
        with pytest.raises(ValueError, match="batch_size"):
            select_batch_kb(None, None, None, None, None, None, None, None, 0, None, None, q)
    with pytest.raises(ValueError, match="unknown form"):
        select_batch_kb(None, None, None, None, None, None, None, None, 0, None, None, 3, form="lds")


def test_reference_spreads_the_batch():
    """On the bucb tests' grid case the believer's picks lie farther apart than the whole top-5 of
    the plain EHVI array spans (measured with a stand-in decomposition: 5.10 against 2.24 grid
    steps); pick 1 is the arg-max of that array and the believed vectors are the means there."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import kb_ref as R
    from test_gpu_bucb import grid_case
    case = grid_case(24, 1)
    pts, y = case["pts"], case["y"]
    ref_point = y.min(axis=0) - 0.5
    ref = R.kb_reference(case["x"], y, pts, case["pm"], case["pv"], case["ls"], 1e-6, 1e-10, 5, case["excluded"],
                         R.pareto_front(y), ref_point)
    idx = ref["idx"]
    assert len(set(idx)) == 5 and idx.min() >= 0 and not case["excluded"][idx].any()

    def pairwise(i):
        d = pts[i][:, None, :] - pts[i][None, :, :]
        return np.sqrt((d * d).sum(-1))[np.triu_indices(len(i), 1)]

    acq = np.where(case["excluded"], -np.inf, ref["acq_first"])
    top5 = np.argsort(-acq, kind="stable")[:5]
    print("believer min distance", pairwise(idx).min(), "top-5 max distance", pairwise(top5).max(),
          "values", ref["val"])
    assert pairwise(idx).min() > pairwise(top5).max()
    assert idx[0] == top5[0]
    np.testing.assert_array_equal(ref["believed"], ref["mu"][:, idx].T)
    assert np.all(ref["val"][1:] < ref["val"][0]) and np.all(ref["val"] > 0)

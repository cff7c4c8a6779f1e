"""The hallucinated-observation batch (GP-BUCB) without a GPU: the descriptor's layout, the
workspace-size query's argument checks and the option's validation (no kernel is launched)."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bucb_desc_layout_matches_header():
    """ctypes mirror of bo_bucb_desc has the C layout (checked against offsetof via a tiny C
    program compiled with gcc)."""
    import subprocess
    import tempfile
    from bayesopt_smart_amd import _lib
    fields = [f for f, _ in _lib.BucbDesc._fields_]
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"bo_amd.h\"\nint main(){\n"
    prog += 'printf("%zu\\n", sizeof(bo_bucb_desc));\n'
    for f in fields:
        prog += f'printf("%zu\\n", offsetof(bo_bucb_desc, {f}));\n'
    prog += "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        vals = [int(v) for v in subprocess.check_output([exe]).split()]
    assert vals[0] == ctypes.sizeof(_lib.BucbDesc)
    for f, off in zip(fields, vals[1:]):
        assert getattr(_lib.BucbDesc, f).offset == off, f


def _desc():
    from bayesopt_smart_amd import _lib
    d = _lib.BucbDesc()
    d.n_obj, d.dim, d.n_train, d.ld_k = 2, 2, 512, 512
    d.cand_kind, d.q, d.n_cand, d.ld = _lib.CAND_GRID, 3, 1 << 20, 1 << 20
    d.grid_shape[0] = d.grid_shape[1] = 1024
    for o in range(2):
        d.prior_var[o], d.length_scale[o], d.beta[o] = 1.0, 30.0, 2.0
    d.jitter, d.min_variance = 1e-6, 1e-10
    return d


def test_workspace_size_query():
    from bayesopt_smart_amd import _lib
    lib = _lib.load()
    size = lambda d: lib.bo_select_batch_bucb_workspace_size(ctypes.byref(d))  # noqa: E731
    d = _desc()
    base = size(d)
    # without var_out the running variance lives in the workspace; never (q - 1) n_obj n_cand doubles
    assert 2 * (1 << 20) * 8 <= base < 2 * 2 * (1 << 20) * 8
    d.var_out = 4096                                     # any non-NULL pointer: sizes only
    assert 0 < size(d) < base - 2 * (1 << 20) * 8 + 4096
    assert lib.bo_select_batch_bucb_workspace_size(None) == 0
    for field, bad in [("q", 0), ("q", 49), ("n_obj", 9), ("n_obj", 0), ("dim", 9), ("n_train", 0),
                       ("ld_k", 511), ("n_cand", 0), ("ld", (1 << 20) - 1), ("cand_kind", 4),
                       ("cand_offset", 1), ("jitter", float("nan")), ("min_variance", -1.0)]:
        d = _desc()
        setattr(d, field, bad)
        assert size(d) == 0, (field, bad)
    d = _desc()
    d.prior_var[1] = 0.0
    assert size(d) == 0
    d = _desc()
    d.length_scale[0] = float("nan")
    assert size(d) == 0
    # the call checks its arguments before it touches the device
    d = _desc()
    d.q = 49
    assert lib.bo_select_batch_bucb(ctypes.byref(d), None, 0, None) == _lib.ERR_ARG
    assert lib.bo_select_batch_bucb(ctypes.byref(_desc()), None, 0, None) == _lib.ERR_ARG   # NULL arrays


def test_batch_strategy_validation():
    from bayesopt_smart_amd import _lib
    from bayesopt_smart_amd.bayesian_optimization import _check_batch_strategy, _check_limits
    _check_batch_strategy("top", "hvi", 1000)
    _check_batch_strategy("bucb", "sum_ucb", _lib.MAX_TOPQ)
    with pytest.raises(ValueError, match="unknown batch_strategy"):
        _check_batch_strategy("believer", "sum_ucb", 3)
    with pytest.raises(ValueError, match="hvi"):
        _check_batch_strategy("bucb", "hvi", 3)
    with pytest.raises(ValueError, match="batch_size <= 48"):
        _check_batch_strategy("bucb", "sum_ucb", _lib.MAX_TOPQ + 1)
    with pytest.raises(ValueError, match="batch_size <= 48"):
        _check_limits(2, 2, 200, 49, "sum_ucb", "bucb")
    with pytest.raises(ValueError, match="unknown batch_strategy"):
        _check_limits(2, 2, 20, 3, "sum_ucb", "thompson")


def test_bucb_rejects_several_ranks(monkeypatch):
    """With collectives on (more than one rank) the option is refused before anything runs."""
    from bayesopt_smart_amd import distributed
    from bayesopt_smart_amd.bayesian_optimization import _check_batch_strategy
    monkeypatch.setattr(distributed, "collectives_on", lambda group=None: True)
    with pytest.raises(ValueError, match="one rank"):
        _check_batch_strategy("bucb", "sum_ucb", 3)
    _check_batch_strategy("top", "sum_ucb", 3)


def test_select_batch_bucb_rejects_bad_batch_size():
    from bayesopt_smart_amd import _lib
    from bayesopt_smart_amd.acquisition import select_batch_bucb
    for q in (0, _lib.MAX_TOPQ + 1):
        with pytest.raises(ValueError, match="batch_size"):
            select_batch_bucb(None, None, None, None, None, None, None, None, None, q)


def test_reference_is_the_conditioned_posterior():
    """tests/bucb_ref.py against the definition's recursion (the stored-v form) in numpy: the two
    agree far below the tests' tolerance, and the picks are identical."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bucb_ref as R
    rng = np.random.default_rng(1)
    ax = np.arange(20.0)
    pts = np.stack([m.ravel() for m in np.meshgrid(ax, ax, indexing="ij")], axis=-1)
    x = pts[rng.choice(400, 15, replace=False)]
    y = np.sin(x / 4.0) @ np.array([[1.0, 0.3], [0.5, 1.0]])
    pm, pv, ls, beta = y.mean(0), np.array([1.3, 0.7]), np.array([4.0, 6.0]), np.array([2.0, 2.0])
    excluded = (pts[:, None, :] == x[None, :, :]).all(-1).any(-1)
    ref = R.bucb_reference(x, y, pts, pm, pv, ls, beta, 1e-6, 1e-10, 5, excluded)
    kinv, cond = R.fitted_state(x, y, pm, pv, ls, 1e-6)
    assert cond.max() < 1e6
    var = ref["var0"].copy()
    vs = [[] for _ in pv]
    for t in range(5):
        acq = R.acquisition(ref["smu"], var, pv, beta)
        p, _ = R.best(acq, ~excluded & ~np.isin(np.arange(400), ref["idx"][:t]))
        assert p == ref["idx"][t]
        for o in range(2):
            ks = R.rbf(pts, x, pv[o], ls[o])
            c = R.rbf(pts, pts[[p]], pv[o], ls[o])[:, 0] - ks @ (kinv[o] @ ks[p])
            for v in vs[o]:
                c = c - v * v[p]
            v = c / np.sqrt(max(c[p], 0.0) + 1e-6)
            vs[o].append(v)
            var[o] = np.maximum(var[o] - v * v, 1e-10)
    assert np.abs(var - ref["var"]).max() <= 1e-9 * pv.max()

"""The Thompson-sampling batch without a GPU: tests/ts_ref.py (the reference the GPU tests compare
against) pinned to the facts that follow from the definition, the option's validation, the
descriptor's layout and the argument checks of the C entry points (no kernel is launched)."""
import ctypes
import functools
import os

import numpy as np
import pytest

import ts_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PV, LS, LAM, N = 1.3, 4.0, 1e-6, 24


def grid_points(lo, shape):
    ax = [np.arange(l, l + s) for l, s in zip(lo, shape)]
    return np.stack([m.ravel() for m in np.meshgrid(*ax, indexing="ij")], axis=-1).astype(np.float64)


@functools.lru_cache(maxsize=None)
def case(n_feat, seed=3):
    pts = grid_points((-5, 100), (33, 31))
    rng = np.random.default_rng(seed)
    x = pts[rng.choice(pts.shape[0], N, replace=False)]
    y = np.sin(x[:, 0] / 5.0) + np.cos(x[:, 1] / 7.0) + 0.05 * rng.standard_normal(N)
    z = rng.standard_normal((n_feat, 2))
    b = rng.uniform(0, 2 * np.pi, n_feat)
    kinv, cond = T.fitted_state(x, [PV], [LS], LAM)
    return dict(pts=pts, x=x, y=y, pm=float(y.mean()), z=z, b=b, kinv=kinv[0], cond=cond[0])


def test_mean_and_variance_over_4000_draws():
    """For fixed (Z, B) the draws' mean is the posterior mean and their variance the closed form."""
    c = case(256)
    n_s = 4000
    rng = np.random.default_rng(12)
    theta = rng.standard_normal((n_s, 256))
    eps = rng.standard_normal((n_s, N))
    f = T.draws_f64(c["x"], c["y"], c["pts"], c["pm"], PV, LS, LAM, c["z"], c["b"], theta, eps, c["kinv"])
    mean, var = T.closed_form(c["x"], c["y"], c["pts"], c["pm"], PV, LS, LAM, c["z"], c["b"], c["kinv"])
    se = np.sqrt(var / n_s)
    worst_mean = (np.abs(f.mean(axis=0) - mean) / se).max()
    worst_var = (np.abs(f.var(axis=0, ddof=1) - var) / (var * np.sqrt(2.0 / (n_s - 1)))).max()
    print("worst mean / se", worst_mean, "worst var / se", worst_var)
    assert worst_mean <= 5.0
    assert worst_var <= 6.0
    # the closed-form variance approximates the exact posterior variance
    k = T.rbf(c["pts"], c["x"], PV, LS)
    exact = PV - np.einsum("mn,nk,mk->m", k, c["kinv"], k)
    assert np.abs(var - exact).max() <= 0.25 * PV


def test_f64_mirror_agrees_with_the_extended_reference():
    """draws_f64 (the statistics' plain numpy form) against reference() under its own bound."""
    c = case(256)
    rng = np.random.default_rng(5)
    theta = rng.standard_normal((3, 1, 256))
    eps = rng.standard_normal((3, 1, N))
    draws = (c["z"][None], c["b"][None], theta, eps)
    ref = T.reference(c["x"], c["y"][:, None], c["pts"], [c["pm"]], [PV], [LS], LAM, draws, c["kinv"][None])
    f = T.draws_f64(c["x"], c["y"], c["pts"], c["pm"], PV, LS, LAM, c["z"], c["b"], theta[:, 0], eps[:, 0],
                    c["kinv"])
    k = T.rbf(c["pts"], c["x"], PV, LS)[ref["sel"]]
    tol = ref["tol_f"][:, 0] + ref["tol_v"][:, 0] @ k.T + 4 * T.U * abs(c["pm"])
    assert (np.abs(f[:, ref["sel"]] - c["pm"] - ref["fc"][:, 0]) <= 4 * tol).all()


@pytest.mark.parametrize("n_feat", [256, 1024])
def test_feature_gram_approximates_the_kernel(n_feat):
    c = case(n_feat)
    phi = T.features_f64(c["x"], c["x"][0], c["z"], c["b"], PV, LS)
    err = np.abs(phi @ phi.T - T.rbf(c["x"], c["x"], PV, LS)).max()
    print("max |Phi Phi^T - K0| / pv", err / PV, "bound", 5 / np.sqrt(n_feat))
    assert err <= 5 * PV / np.sqrt(n_feat)


def test_training_point_identity():
    """f(x_n) = y_n - sqrt(lam) E_n - lam v_n, because K0 v = r - lam v."""
    c = case(256)
    rng = np.random.default_rng(7)
    theta = rng.standard_normal((4, 1, 256))
    eps = rng.standard_normal((4, 1, N))
    draws = (c["z"][None], c["b"][None], theta, eps)
    ref = T.reference(c["x"], c["y"][:, None], c["x"], [c["pm"]], [PV], [LS], LAM, draws, c["kinv"][None])
    sel = ref["sel"]
    want = c["y"][None, sel] - np.sqrt(LAM) * eps[:, 0][:, sel] - LAM * ref["v"][:, 0][:, sel]
    err = np.abs(c["pm"] + ref["fc"][:, 0] - want).max()
    print("identity error", err, "cond", c["cond"])
    assert err <= 1e-12


def test_constants_within_the_cap():
    for n, d, dim in [(1, 1, 1), (24, 37, 2), (1024, 1024, 6), (65536, 1, 8)]:
        cf, cv = T.constants(n, d, dim)
        assert cf == n + d + 2 * dim + 16 and cv <= cf + 64


# ------------------------------------------------------------------------- options and the ABI
def test_ts_strategy_validation(monkeypatch):
    from bayesopt_smart_amd import _lib, distributed
    from bayesopt_smart_amd.acquisition import BATCH_STRATEGIES
    from bayesopt_smart_amd.bayesian_optimization import _check_batch_strategy, _check_limits
    assert BATCH_STRATEGIES == ("top", "bucb", "ts")
    _check_batch_strategy("ts", "sum_ucb", _lib.MAX_TOPQ)
    _check_batch_strategy("ts", "hvi", 4)
    _check_limits(2, 2, 60, 4, "hvi", "ts")
    with pytest.raises(ValueError, match="no sampled form"):
        _check_batch_strategy("ts", "ehvi", 3)
    with pytest.raises(ValueError, match="batch_size <= 48"):
        _check_batch_strategy("ts", "sum_ucb", 49)
    with pytest.raises(ValueError, match="at most 4 objectives"):
        _check_limits(5, 2, 60, 4, "hvi", "ts")
    with pytest.raises(ValueError, match=r"unknown batch_strategy.*'top', 'bucb' or 'ts'"):
        _check_batch_strategy("thompson", "sum_ucb", 3)
    monkeypatch.setattr(distributed, "collectives_on", lambda group=None: True)
    _check_batch_strategy("ts", "sum_ucb", 3)                    # several ranks are fine
    _check_batch_strategy("ts", "hvi", 3)


def test_thompson_draws_leaves_the_global_rng_alone():
    from bayesopt_smart_amd.acquisition import thompson_draws
    np.random.seed(42)
    before = np.random.get_state()
    z, b, theta, eps = thompson_draws(np.random.default_rng(1), 2, 3, 10, 4, 37)
    after = np.random.get_state()
    assert before[0] == after[0] and (before[1] == after[1]).all() and before[2:] == after[2:]
    assert z.shape == (2, 37, 3) and b.shape == (2, 37) and theta.shape == (4, 2, 37) and eps.shape == (4, 2, 10)
    assert (b >= 0).all() and (b < 2 * np.pi).all()
    again = thompson_draws(np.random.default_rng(1), 2, 3, 10, 4, 37)
    assert all((p == q).all() for p, q in zip((z, b, theta, eps), again))
    with pytest.raises(TypeError):
        thompson_draws(np.random, 2, 3, 10, 4, 37)


def test_resolve_ts_picks():
    from bayesopt_smart_amd.acquisition import resolve_ts_picks
    got = resolve_ts_picks([[5], [5, 7], [5, 7, -1], [9, -1, -1, -1]])
    assert got.tolist() == [5, 7, -1, 9]


def test_ts_desc_layout_matches_header():
    import subprocess
    import tempfile
    from bayesopt_smart_amd import _lib
    fields = [f for f, _ in _lib.TsDesc._fields_]
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"bo_amd.h\"\nint main(){\n"
    prog += 'printf("%zu\\n", sizeof(bo_ts_desc));\nprintf("%d\\n", BO_TS_MAX_FEATURES);\n'
    for f in fields:
        prog += f'printf("%zu\\n", offsetof(bo_ts_desc, {f}));\n'
    prog += "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        vals = [int(v) for v in subprocess.check_output([exe]).split()]
    assert vals[0] == ctypes.sizeof(_lib.TsDesc)
    assert vals[1] == _lib.TS_MAX_FEATURES
    for f, off in zip(fields, vals[2:]):
        assert getattr(_lib.TsDesc, f).offset == off, f


def _desc():
    from bayesopt_smart_amd import _lib
    d = _lib.TsDesc()
    d.n_obj, d.dim, d.n_train, d.ld_k, d.ld_y = 2, 2, 512, 512, 2
    d.cand_kind, d.n_samples, d.n_features, d.n_cand, d.ld = _lib.CAND_GRID, 3, 1000, 1 << 20, 1 << 20
    d.grid_shape[0] = d.grid_shape[1] = 1024
    for o in range(2):
        d.prior_mean[o], d.prior_var[o], d.length_scale[o] = 0.5, 1.0, 30.0
    d.jitter = 1e-6
    return d


def test_workspace_size_query_and_argument_checks():
    from bayesopt_smart_amd import _lib
    lib = _lib.load()
    size = lambda d: lib.bo_sample_paths_workspace_size(ctypes.byref(d))  # noqa: E731
    base = size(_desc())
    # nothing N x M and nothing candidate-sized: rows, the weight matrix, the right-hand sides
    assert 0 < base < 2 * (1000 + 512 + 8) * (16 + 3) * 8 + 3 * 2 * 512 * 8 + 8 * 256
    assert lib.bo_sample_paths_workspace_size(None) == 0
    for field, bad in [("n_samples", 0), ("n_samples", 49), ("n_features", 0),
                       ("n_features", _lib.TS_MAX_FEATURES + 1), ("n_obj", 9), ("n_obj", 0), ("dim", 9), ("dim", 0),
                       ("n_train", 0), ("ld_k", 511), ("ld_y", 1), ("n_cand", 0), ("ld", (1 << 20) - 1),
                       ("cand_kind", 4), ("cand_offset", 1), ("cand_offset", -1), ("jitter", float("nan")),
                       ("jitter", -1.0)]:
        d = _desc()
        setattr(d, field, bad)
        assert size(d) == 0, (field, bad)
    for arr, bad in [("prior_var", 0.0), ("length_scale", float("nan")), ("prior_mean", float("inf"))]:
        d = _desc()
        getattr(d, arr)[1] = bad
        assert size(d) == 0, arr
    d = _desc()
    d.n_features = 1001                                    # any value, not only multiples of 4
    assert size(d) >= base
    # the call checks its arguments before it touches the device
    d = _desc()
    d.n_samples = 49
    assert lib.bo_sample_paths(ctypes.byref(d), None, 0, None) == _lib.ERR_ARG
    assert lib.bo_sample_paths(ctypes.byref(_desc()), None, 0, None) == _lib.ERR_ARG        # NULL arrays
    assert {"bo_sample_paths", "bo_sample_paths_workspace_size"} <= set(_lib.symbols())


def test_select_batch_ts_rejects_bad_options():
    from bayesopt_smart_amd.acquisition import select_batch_ts
    with pytest.raises(ValueError, match="no sampled form"):
        select_batch_ts(None, None, None, None, None, None, None, None, None, 3, acquisition="ehvi")
    for q in (0, 49):
        with pytest.raises(ValueError, match="batch_size"):
            select_batch_ts(None, None, None, None, None, None, None, None, None, q)

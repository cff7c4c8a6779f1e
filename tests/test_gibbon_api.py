"""The GIBBON batch (batch_strategy="gibbon", bo_select_batch_gibbon) without a GPU: what the
constructor's limit check accepts and refuses, the strategy tuples, the descriptor's layout, and the
entry point's argument checks, which run before the device is touched (no kernel is launched)."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x1000          # a non-NULL, 16-byte aligned pointer that is never dereferenced: every call below fails its checks


def limits(**kw):
    from bayesopt_smart_amd.bayesian_optimization import _check_limits
    args = dict(n_obj=5, dim=2, total_samples=40, batch_size=3, acquisition="mes", batch_strategy="gibbon")
    args.update(kw)
    return _check_limits(**args)


# ------------------------------------------------------------------ the option's validation
@pytest.mark.parametrize("n_obj", [1, 5, 8])
def test_limits_accept_gibbon(n_obj):
    from bayesopt_smart_amd import _lib
    limits(n_obj=n_obj)
    limits(n_obj=n_obj, batch_size=1)
    limits(n_obj=n_obj, batch_size=_lib.MAX_TOPQ, total_samples=8 + 2 * _lib.MAX_TOPQ)
    limits(n_obj=n_obj, batch_strategy="top", batch_size=60)        # "top" keeps its rounds above BO_MAX_TOPQ


def test_limits_reject_large_batch():
    with pytest.raises(ValueError, match=r"batch_strategy='gibbon' supports batch_size <= 48 \(got 49\)"):
        limits(batch_size=49, total_samples=200)


@pytest.mark.parametrize("acquisition", ["sum_ucb", "hvi", "ehvi"])
def test_limits_reject_other_acquisitions(acquisition):
    with pytest.raises(ValueError, match="batch correction of an information criterion") as e:
        limits(n_obj=2, acquisition=acquisition)
    assert "acquisition='mes' only" in str(e.value) and repr(acquisition) in str(e.value)


def test_limits_reject_several_ranks(monkeypatch):
    from bayesopt_smart_amd import distributed
    monkeypatch.setattr(distributed, "collectives_on", lambda group=None: True)
    with pytest.raises(ValueError, match="one rank.*all-gather of the per-rank best candidates"):
        limits()
    limits(batch_strategy="top")                                     # "mes" itself runs on any number of ranks


def test_limits_reject_constraints():
    with pytest.raises(ValueError, match="outcome constraints need"):
        limits(n_obj=2, n_constraints=1, constraint_bounds=[(0.0, 1.0)])
    with pytest.raises(ValueError, match="outcome constraints need batch_strategy='top'"):
        limits(n_obj=2, acquisition="ehvi", n_constraints=1, constraint_bounds=[(0.0, 1.0)])


def test_other_strategies_point_to_gibbon():
    for strategy in ("bucb", "ts", "kb"):
        with pytest.raises(ValueError, match="acquisition='mes' supports batch_strategy='top' only") as e:
            limits(batch_strategy=strategy)
        assert "conditioned on the earlier picks" in str(e.value) and "'gibbon'" in str(e.value)
    with pytest.raises(ValueError, match=r"unknown batch_strategy 'believer'.*acquisition='ehvi'\), or 'gibbon' with "
                                         r"acquisition='mes'"):
        limits(batch_strategy="believer")


def test_tuples():
    from bayesopt_smart_amd import acquisition
    assert acquisition.MES_BATCH_STRATEGIES == ("top", "gibbon")
    assert acquisition.BATCH_STRATEGIES == ("top", "bucb", "ts")          # the pinned tuples are unchanged
    assert acquisition.ALL_BATCH_STRATEGIES == ("top", "bucb", "ts", "kb")


def test_python_entry_points_check_before_the_device():
    from bayesopt_smart_amd import _lib
    from bayesopt_smart_amd.acquisition import mes_select_indices, select_batch_gibbon
    for q in (0, _lib.MAX_TOPQ + 1):
        with pytest.raises(ValueError, match="batch_size"):
            select_batch_gibbon(None, None, None, None, None, None, None, None, q)
    with pytest.raises(ValueError, match="unknown batch_strategy 'bucb' for the max-value entropy"):
        mes_select_indices(None, None, None, None, None, None, None, None, None, None, None, None, 3,
                           batch_strategy="bucb")


def test_symbols():
    from bayesopt_smart_amd import _lib
    assert {"bo_select_batch_gibbon", "bo_select_batch_gibbon_workspace_size"} <= set(_lib.symbols())
    lib = _lib.load()
    assert lib.bo_abi_version() == 5                                    # additive: the ABI version stays
    assert lib.bo_select_batch_gibbon.argtypes[0]._type_ is _lib.GibbonDesc


# ------------------------------------------------------------------ the descriptor and the C entry
def test_gibbon_desc_layout_matches_header():
    """The ctypes mirror of bo_gibbon_desc has the C layout (offsetof via a tiny C program)."""
    import subprocess
    import tempfile
    from bayesopt_smart_amd import _lib
    fields = [f for f, _ in _lib.GibbonDesc._fields_]
    assert "beta" not in fields and "std_mu" not in fields
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"bo_amd.h\"\nint main(){\n"
    prog += 'printf("%zu\\n", sizeof(bo_gibbon_desc));\n'
    for f in fields:
        prog += f'printf("%zu\\n", offsetof(bo_gibbon_desc, {f}));\n'
    prog += "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        with open(c, "w") as fh:
            fh.write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        vals = [int(v) for v in subprocess.check_output([exe]).split()]
    assert vals[0] == ctypes.sizeof(_lib.GibbonDesc)
    for f, off in zip(fields, vals[1:]):
        assert getattr(_lib.GibbonDesc, f).offset == off, f


def desc(**kw):
    """A descriptor every check accepts (the pointers are never dereferenced)."""
    from bayesopt_smart_amd import _lib
    d = _lib.GibbonDesc()
    d.n_obj, d.dim, d.n_train, d.ld_k = 5, 2, 512, 512
    d.cand_kind, d.q, d.n_cand, d.ld = _lib.CAND_GRID, 3, 1 << 20, 1 << 20
    d.grid_shape[0] = d.grid_shape[1] = 1024
    for o in range(5):
        d.prior_var[o], d.length_scale[o] = 1.0, 30.0
    d.jitter, d.min_variance = 1e-6, 1e-10
    d.x_train, d.kinv, d.base, d.var, d.top_val, d.top_idx = P, P + 0x1000, P + 0x2000, P + 0x3000, P + 0x4000, P + 0x5000
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def size(d):
    from bayesopt_smart_amd import _lib
    return _lib.load().bo_select_batch_gibbon_workspace_size(ctypes.byref(d))


def call(d, ws=P, ws_bytes=None):
    from bayesopt_smart_amd import _lib
    return _lib.load().bo_select_batch_gibbon(ctypes.byref(d), ws, size(d) if ws_bytes is None else ws_bytes, None)


def test_workspace_size_query():
    from bayesopt_smart_amd import _lib
    lib = _lib.load()
    base = size(desc())
    # without var_out the running variance lives in the workspace; nothing else is candidate-sized
    # beyond the mask and the per-workgroup bests: never (q - 1) n_obj n_cand doubles
    assert 5 * (1 << 20) * 8 <= base < 6 * (1 << 20) * 8
    assert 0 < size(desc(var_out=P + 0x6000)) < base - 5 * (1 << 20) * 8 + 4096
    assert lib.bo_select_batch_gibbon_workspace_size(None) == 0
    # the workspace is the hallucinated-observation update's: the same bytes as "bucb" for the same shapes
    b = _lib.BucbDesc()
    g = desc()
    for f, _ in _lib._UPDATE_FIELDS:
        setattr(b, f, getattr(g, f))
    b.jitter, b.min_variance, b.ld = g.jitter, g.min_variance, g.ld
    assert lib.bo_select_batch_bucb_workspace_size(ctypes.byref(b)) == base


BAD_FIELDS = [("q", 0), ("q", 49), ("n_obj", 9), ("n_obj", 0), ("dim", 9), ("dim", 0), ("n_train", 0), ("ld_k", 511),
              ("n_cand", 0), ("ld", (1 << 20) - 1), ("cand_kind", 4), ("cand_kind", -1), ("cand_offset", 1),
              ("cand_offset", -1), ("jitter", float("nan")), ("jitter", -1.0), ("jitter", float("inf")),
              ("min_variance", -1.0), ("min_variance", float("nan"))]


@pytest.mark.parametrize("field,bad", BAD_FIELDS)
def test_bad_fields_are_refused(field, bad):
    from bayesopt_smart_amd import _lib
    d = desc(**{field: bad})
    assert size(d) == 0
    assert call(d, ws_bytes=1 << 30) == _lib.ERR_ARG


def test_bad_hyperparameters_are_refused():
    from bayesopt_smart_amd import _lib
    for arr, bad in [("prior_var", 0.0), ("prior_var", float("inf")), ("prior_var", float("nan")),
                     ("length_scale", 0.0), ("length_scale", float("nan"))]:
        d = desc()
        getattr(d, arr)[4] = bad
        assert size(d) == 0 and call(d, ws_bytes=1 << 30) == _lib.ERR_ARG, (arr, bad)
        d = desc()
        getattr(d, arr)[5] = bad                                       # entries past n_obj are not read
        assert size(d) > 0
    d = desc()
    d.grid_shape[1] = 1023                                             # the shard no longer fits the grid
    assert size(d) == 0 and call(d, ws_bytes=1 << 30) == _lib.ERR_ARG


def test_null_and_aliased_pointers_are_refused():
    from bayesopt_smart_amd import _lib
    E = _lib.ERR_ARG
    assert _lib.load().bo_select_batch_gibbon(None, P, 1 << 30, None) == E
    for f in ("x_train", "kinv", "base", "var", "top_val", "top_idx"):
        assert call(desc(**{f: None})) == E, f
    assert call(desc(cand_kind=_lib.CAND_F64, cand=None)) == E        # explicit candidates need their rows
    assert call(desc(cand_kind=_lib.CAND_I64, cand=None)) == E
    d = desc()
    for out, inp in [("var_out", "var"), ("var_out", "base"), ("acq_last", "base"), ("acq_last", "var")]:
        assert call(desc(**{out: getattr(d, inp)})) == E, (out, inp)   # the inputs stay as they are
    assert call(desc(var_out=P + 0x6000, acq_last=P + 0x6000)) == E   # two outputs in one buffer
    assert call(desc(), ws=P + 8) == E                                 # the workspace is 16-byte aligned


def test_workspace_is_checked():
    from bayesopt_smart_amd import _lib
    d = desc()
    assert call(d, ws=None) == _lib.ERR_WORKSPACE
    assert call(d, ws=None, ws_bytes=0) == _lib.ERR_WORKSPACE
    assert call(d, ws_bytes=size(d) - 1) == _lib.ERR_WORKSPACE
    # optional outputs stay optional: with them the argument checks pass too, and the short
    # workspace is what is reported
    assert call(desc(var_out=P + 0x6000, acq_last=P + 0x7000), ws_bytes=64) == _lib.ERR_WORKSPACE

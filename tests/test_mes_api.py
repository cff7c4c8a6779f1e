"""Acquisition "mes" without a device: what the constructor's limit check accepts and refuses, and the
argument checks of bo_path_maxima / bo_max_value_entropy, which run before the device is touched."""
import ctypes

import numpy as np
import pytest


def limits(**kw):
    from bayesopt_smart_amd.bayesian_optimization import _check_limits
    args = dict(n_obj=5, dim=2, total_samples=40, batch_size=3, acquisition="mes")
    args.update(kw)
    return _check_limits(**args)


@pytest.mark.parametrize("n_obj", [1, 5, 8])
def test_limits_accept_mes(n_obj):
    limits(n_obj=n_obj)
    limits(n_obj=n_obj, mes_samples=1)
    limits(n_obj=n_obj, mes_samples=48)
    limits(n_obj=n_obj, batch_size=60)             # above BO_MAX_TOPQ: the rounds of select_indices


def test_mes_is_a_known_acquisition():
    from bayesopt_smart_amd import bayesian_optimization as B
    assert "mes" in B.ACQUISITIONS
    B._check_acquisition("mes")
    with pytest.raises(ValueError, match="unknown acquisition"):
        B._check_acquisition("pes")


@pytest.mark.parametrize("s", [0, 49, -1])
def test_limits_reject_mes_samples(s):
    with pytest.raises(ValueError, match="mes_samples"):
        limits(mes_samples=s)
    limits(acquisition="sum_ucb", mes_samples=s)   # only "mes" reads it


def test_limits_reject_nine_objectives():
    with pytest.raises(ValueError, match="n_objectives"):
        limits(n_obj=9)


@pytest.mark.parametrize("strategy", ["bucb", "ts", "kb"])
def test_limits_reject_other_batch_strategies(strategy):
    with pytest.raises(ValueError, match="acquisition='mes' supports batch_strategy='top' only") as e:
        limits(batch_strategy=strategy)
    assert repr(strategy) in str(e.value) and "conditioned on the earlier picks" in str(e.value)


def test_other_acquisitions_keep_their_ts_message():
    with pytest.raises(ValueError) as e:
        limits(n_obj=2, acquisition="ehvi", batch_strategy="ts")
    assert str(e.value) == ("batch_strategy='ts' scores posterior draws; acquisition='ehvi' integrates over "
                            "the posterior and has no sampled form (got acquisition='ehvi')")


def test_limits_reject_constraints():
    with pytest.raises(ValueError, match="outcome constraints need acquisition='ehvi'"):
        limits(n_obj=2, n_constraints=1, constraint_bounds=[(0.0, 1.0)])


# ------------------------------------------------------------------ the C entries' argument checks
P = 0x1000          # a non-NULL pointer that is never dereferenced: every call below fails its checks


def vec(*v):
    return (ctypes.c_double * 8)(*(list(v) + [1.0] * (8 - len(v))))


def maxima(ystar=P, paths=P, ld=10, n_cand=10, n_s=2, n_obj=2, shift=None, scale=None, ws=P, ws_bytes=1 << 20):
    from bayesopt_smart_amd import _lib
    return _lib.load().bo_path_maxima(ystar, paths, ld, n_cand, n_s, n_obj, shift if shift is not None else vec(0.0, 0.0),
                                      scale if scale is not None else vec(1.0, 1.0), ws, ws_bytes, None)


def scan(acq=P, mu=P, var=P, ld=10, n=10, n_obj=2, ystar=P, n_s=2):
    from bayesopt_smart_amd import _lib
    return _lib.load().bo_max_value_entropy(acq, mu, var, ld, n, n_obj, ystar, n_s, None)


def test_path_maxima_argument_checks():
    from bayesopt_smart_amd import _lib
    E = _lib.ERR_ARG
    assert maxima(ystar=None) == E and maxima(paths=None) == E
    assert maxima(shift=ctypes.POINTER(ctypes.c_double)()) == E and maxima(scale=ctypes.POINTER(ctypes.c_double)()) == E
    assert maxima(n_obj=0) == E and maxima(n_obj=9) == E
    assert maxima(n_s=0) == E and maxima(n_s=49) == E
    assert maxima(ld=9) == E and maxima(n_cand=-1, ld=0) == E
    for bad in (0.0, -1.0, np.inf, np.nan):
        assert maxima(scale=vec(1.0, bad)) == E, bad
    for bad in (np.inf, -np.inf, np.nan):
        assert maxima(shift=vec(0.0, bad)) == E, bad
    assert maxima(scale=vec(1.0, 1.0, -1.0), ws=None) == _lib.ERR_WORKSPACE    # entries past n_obj are not read
    assert maxima(ws=None) == _lib.ERR_WORKSPACE and maxima(ws_bytes=8) == _lib.ERR_WORKSPACE


def test_path_maxima_workspace_size():
    from bayesopt_smart_amd import _lib
    lib = _lib.load()
    assert lib.bo_path_maxima_workspace_size(-1, 4) == 0
    assert lib.bo_path_maxima_workspace_size(10, 0) == 0 and lib.bo_path_maxima_workspace_size(10, 385) == 0
    small, big = lib.bo_path_maxima_workspace_size(0, 1), lib.bo_path_maxima_workspace_size(1 << 21, 384)
    assert small > 0 and small % 256 == 0 and big % 256 == 0
    assert 384 * ((1 << 21) // 8192) * 8 <= big < 4 << 20          # one double per row and 8192 columns


def test_max_value_entropy_argument_checks():
    from bayesopt_smart_amd import _lib
    E = _lib.ERR_ARG
    assert scan(acq=None) == E and scan(mu=None) == E and scan(var=None) == E and scan(ystar=None) == E
    assert scan(n_obj=0) == E and scan(n_obj=9) == E
    assert scan(n_s=0) == E and scan(n_s=49) == E
    assert scan(ld=9) == E and scan(n=-1) == E
    assert scan(n=0, ld=0) == _lib.OK                # nothing to do, nothing launched

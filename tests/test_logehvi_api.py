"""Acquisition "logehvi" without a device: what the constructor's limit check accepts and refuses, the
argument checks of bo_log_ehvi (all before the device is touched) and the table form's admission
rule against its Python mirror."""
import ctypes

import numpy as np
import pytest

import logehvi_ref as R


def limits(**kw):
    from bayesopt_smart_amd.bayesian_optimization import _check_limits
    args = dict(n_obj=2, dim=2, total_samples=40, batch_size=3, acquisition="logehvi")
    args.update(kw)
    return _check_limits(**args)


def test_logehvi_is_a_known_acquisition():
    from bayesopt_smart_amd import acquisition as A
    from bayesopt_smart_amd import bayesian_optimization as B
    assert "logehvi" in B.ACQUISITIONS
    B._check_acquisition("logehvi")
    with pytest.raises(ValueError, match="unknown acquisition"):
        B._check_acquisition("logei")
    assert callable(A.log_expected_hypervolume_improvement) and callable(A.update_log_expected_hypervolume_improvement)


@pytest.mark.parametrize("n_obj", [1, 2, 4])
def test_limits_accept_logehvi(n_obj):
    limits(n_obj=n_obj)
    limits(n_obj=n_obj, batch_size=60)             # above BO_MAX_TOPQ: the rounds of select_indices
    limits(n_obj=n_obj, n_constraints=1, constraint_bounds=[(0.0, np.inf)])
    limits(n_obj=n_obj, n_constraints=8 - n_obj, constraint_bounds=[(-1.0, 1.0)] * (8 - n_obj))


def test_limits_reject_five_objectives_and_nine_outputs():
    with pytest.raises(ValueError, match="acquisition='logehvi' supports at most 4 objectives"):
        limits(n_obj=5)
    with pytest.raises(ValueError, match="n_objectives \\+ n_constraints must be <= 8"):
        limits(n_obj=4, n_constraints=5, constraint_bounds=[(0.0, 1.0)] * 5)
    with pytest.raises(ValueError, match="exceeds the upper bound"):
        limits(n_constraints=1, constraint_bounds=[(1.0, 0.0)])


@pytest.mark.parametrize("strategy,reason", [("bucb", "conditions the UCB acquisition"),
                                             ("ts", "no sampled form"),
                                             ("kb", "a believer over the log value is not built")])
def test_limits_reject_other_batch_strategies(strategy, reason):
    with pytest.raises(ValueError, match="acquisition='logehvi' supports batch_strategy='top' only") as e:
        limits(batch_strategy=strategy)
    assert repr(strategy) in str(e.value) and reason in str(e.value)


def test_gibbon_keeps_its_reason():
    with pytest.raises(ValueError, match="defined for acquisition='mes' only") as e:
        limits(batch_strategy="gibbon")
    assert "got acquisition='logehvi'" in str(e.value)


def test_other_acquisitions_keep_their_messages():
    with pytest.raises(ValueError) as e:
        limits(acquisition="ehvi", batch_strategy="ts")
    assert str(e.value) == ("batch_strategy='ts' scores posterior draws; acquisition='ehvi' integrates over "
                            "the posterior and has no sampled form (got acquisition='ehvi')")
    with pytest.raises(ValueError, match="outcome constraints need acquisition='ehvi'"):
        limits(acquisition="mes", n_obj=2, n_constraints=1, constraint_bounds=[(0.0, 1.0)])
    with pytest.raises(ValueError, match="defined for acquisition='ehvi' only"):
        limits(acquisition="sum_ucb", batch_strategy="kb")


# ------------------------------------------------------------------ the C entry's argument checks
P = 0x1000          # a non-NULL pointer that is never dereferenced: every call below fails its checks


def vec(*v):
    return (ctypes.c_double * 8)(*(list(v) + [0.0] * (8 - len(v))))


def scan(acq=P, logpof=None, mu=P, var=P, ld=10, n=10, n_obj=2, n_con=0, lo=None, hi=None, boxes=P, n_boxes=3, edges=P,
         n_edges=(2, 2), box_idx=P, form=0):
    from bayesopt_smart_amd import _lib
    ne = (ctypes.c_int32 * 4)(*n_edges) if n_edges is not None else None
    return _lib.load().bo_log_ehvi(acq, logpof, mu, var, ld, n, n_obj, n_con, lo, hi, boxes, n_boxes, edges, ne, box_idx,
                                   form, None)


def test_log_ehvi_argument_checks():
    from bayesopt_smart_amd import _lib
    E, inf, nan = _lib.ERR_ARG, np.inf, np.nan
    # bo_constrained_ehvi's cases
    assert scan(n_con=1, lo=vec(1.0), hi=vec(0.0)) == E                                     # lo > hi
    assert scan(n_con=1, lo=vec(nan), hi=vec(0.0)) == E and scan(n_con=1, lo=vec(0.0), hi=vec(nan)) == E
    assert scan(n_con=1, lo=vec(inf), hi=vec(inf)) == E and scan(n_con=1, lo=vec(-inf), hi=vec(-inf)) == E
    assert scan(n_obj=0) == E and scan(n_obj=5) == E and scan(n_con=-1) == E
    assert scan(n_obj=2, n_con=7, lo=vec(), hi=vec()) == E                                  # 9 outputs
    assert scan(n_con=1, lo=None, hi=vec(0.0)) == E and scan(n_con=1, lo=vec(0.0), hi=None) == E
    # the scan's own
    assert scan(acq=None) == E and scan(mu=None) == E and scan(var=None) == E
    assert scan(ld=9) == E and scan(n=-1) == E and scan(n_boxes=-1) == E
    assert scan(form=-1) == E and scan(form=3) == E
    assert scan(form=1, boxes=None) == E and scan(form=2, n_edges=None) == E and scan(form=2, edges=None) == E
    assert scan(form=0, boxes=None, n_edges=None) == E
    assert scan(form=2, n_edges=(0, 2)) == E                                                # an axis without an edge
    # no table fits: form 2 is unsupported, auto falls back to the direct form only when it has the boxes
    assert scan(form=2, n_edges=(100, 61)) == _lib.ERR_UNSUPPORTED
    assert scan(form=0, boxes=None, n_edges=(100, 61)) == _lib.ERR_UNSUPPORTED
    # nothing to do, nothing launched
    assert scan(n=0, ld=0) == _lib.OK
    assert scan(n=0, ld=0, n_con=1, lo=vec(-inf), hi=vec(inf)) == _lib.OK


def test_table_threads_match_the_mirror():
    from bayesopt_smart_amd import _lib
    lib = _lib.load()
    for s in list(range(-2, 200)) + [319, 320, 321, 1 << 20, 1 << 40]:
        assert lib.bo_logehvi_table_threads(s) == R.table_threads(s), s
    assert lib.bo_logehvi_table_threads(80) == 128 and lib.bo_ehvi_table_threads(80) == 256     # 16 against 8 bytes

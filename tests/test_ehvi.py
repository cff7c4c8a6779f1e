"""Expected hypervolume improvement (acquisition="ehvi"; not in the reference, which has no EHVI:
PARITY UNPINNED), the part that needs no GPU: the numpy closed form of tests/ehvi_ref.py against a
Monte-Carlo mean of the box sum (which tests/test_hvi.py pins against the brute-force hypervolume),
the host edge tables (bo_ehvi_tables), the admission rule's mirror, and the limits."""
import ctypes

import numpy as np
import pytest

import ehvi_ref as R
from test_hvi import _front, _hvi_from_boxes

N_DRAWS = 200_000
N_POSTERIORS = 10


def _mc_cases():
    for m in (1, 2, 3, 4):
        for n in (0, 5, 17):
            for kind in ("cont", "int"):
                if m == 4 and n > 5:
                    continue
                yield m, n, kind


@pytest.mark.parametrize("m,n,kind", list(_mc_cases()))
def test_reference_matches_monte_carlo(m, n, kind):
    """|closed form - MC mean| <= 5 standard errors of that mean (from the draws), for 10 random
    posteriors per front with sigma in [0.05, 2].  A posterior is used only when at least 50 of its
    2e5 draws improve the front: with none the MC mean and its standard error are both 0 and say
    nothing (that regime is covered on the device against this closed form)."""
    from bayesopt_smart_amd.acquisition import hypervolume_boxes
    rng = np.random.default_rng(1000 * m + 10 * n + (kind == "int"))
    front = _front(rng, n, m, kind)
    r = np.full(m, -1.0)
    boxes = hypervolume_boxes(front, r)
    z = rng.standard_normal((N_DRAWS, m))
    used, worst = 0, 0.0
    for _ in range(20 * N_POSTERIORS):
        mu = rng.uniform(-1.0, 6.0, size=m)
        sigma = rng.uniform(0.05, 2.0, size=m)
        hv = _hvi_from_boxes_chunked(boxes, mu + sigma * z)
        if np.count_nonzero(hv) < 50:
            continue
        ref = R.ehvi(mu[:, None], (sigma ** 2)[:, None], boxes)[0]
        se = hv.std(ddof=1) / np.sqrt(N_DRAWS)
        dev = abs(ref - hv.mean()) / se
        worst = max(worst, dev)
        assert dev <= 5.0, (mu, sigma, ref, hv.mean(), se)
        used += 1
        if used == N_POSTERIORS:
            break
    assert used == N_POSTERIORS
    print(f"m={m} n={n} {kind}: worst deviation {worst:.2f} standard errors")


def _hvi_from_boxes_chunked(boxes, pts, chunk=4000):
    return np.concatenate([_hvi_from_boxes(boxes, pts[i:i + chunk]) for i in range(0, pts.shape[0], chunk)])


def test_psi_limits():
    mu = np.array([0.3, -2.0, 5.0])
    assert np.array_equal(R.psi(mu, np.zeros(3), 1.0), np.maximum(mu - 1.0, 0.0))
    assert np.array_equal(R.psi(mu, np.ones(3), np.inf), np.zeros(3))
    # far above the bound psi is mu - a, far below it is 0
    assert R.psi(np.array([50.0]), np.array([1.0]), 0.0)[0] == pytest.approx(50.0, rel=1e-15)
    assert 0.0 <= R.psi(np.array([-50.0]), np.array([1.0]), 0.0)[0] < 1e-300


@pytest.mark.parametrize("m,n,kind", [(m, n, k) for m in (1, 2, 3, 4) for n in (0, 5, 17) for k in ("cont", "int")
                                      if not (m == 4 and n > 5)])
def test_tables_reproduce_every_box_bound(m, n, kind):
    from bayesopt_smart_amd.acquisition import ehvi_tables, hypervolume_boxes
    rng = np.random.default_rng(7 * m + n)
    boxes = hypervolume_boxes(_front(rng, n, m, kind), np.full(m, -1.0))
    edges, idx = ehvi_tables(boxes)
    assert idx.shape == boxes.shape and idx.dtype == np.int32
    assert [len(e) for e in edges] == R.edge_counts(boxes, m)
    for k in range(m):
        assert np.all(np.diff(edges[k]) > 0) and np.all(np.isfinite(edges[k]))
        ext = np.append(edges[k], np.inf)                   # index E_k stands for +inf
        assert np.all((idx[:, k] >= 0) & (idx[:, k] < len(edges[k])))
        assert np.all((idx[:, m + k] >= 0) & (idx[:, m + k] <= len(edges[k])))
        assert np.array_equal(ext[idx[:, k]], boxes[:, k])
        assert np.array_equal(ext[idx[:, m + k]], boxes[:, m + k])
    if n == 0:
        assert boxes.shape[0] == 1 and [len(e) for e in edges] == [1] * m


def test_tables_capacity_retry_and_arguments():
    from bayesopt_smart_amd import _lib
    from bayesopt_smart_amd.acquisition import ehvi_tables, hypervolume_boxes
    lib = _lib.load()
    rng = np.random.default_rng(5)
    t = rng.uniform(0, np.pi / 2, size=70)
    front = np.stack([np.cos(t), np.sin(t)], axis=1)
    boxes = hypervolume_boxes(front, np.zeros(2))
    edges, idx = ehvi_tables(boxes)                         # more edges than the first capacity guess
    need = sum(len(e) for e in edges)
    assert need > 64 and need == sum(R.edge_counts(boxes, 2))
    ne = (ctypes.c_int32 * 2)()
    buf = np.full(need, -7.0)
    got = np.full(idx.shape, -7, dtype=np.int32)
    st = lib.bo_ehvi_tables(boxes.ctypes.data, boxes.shape[0], 2, buf.ctypes.data, need - 1, ne, got.ctypes.data)
    assert st == _lib.ERR_WORKSPACE and list(ne) == [len(e) for e in edges]
    assert np.all(buf == -7.0) and np.all(got == -7)        # one short: the counts and nothing else
    st = lib.bo_ehvi_tables(boxes.ctypes.data, boxes.shape[0], 2, None, 0, ne, None)
    assert st == _lib.ERR_WORKSPACE and sum(ne) == need     # the query
    st = lib.bo_ehvi_tables(boxes.ctypes.data, boxes.shape[0], 2, buf.ctypes.data, need, ne, got.ctypes.data)
    assert st == _lib.OK and np.array_equal(buf, np.concatenate(edges)) and np.array_equal(got, idx)
    # no boxes: no edges
    st = lib.bo_ehvi_tables(None, 0, 3, None, 0, (ctypes.c_int32 * 3)(), None)
    assert st == _lib.OK
    assert lib.bo_ehvi_tables(boxes.ctypes.data, boxes.shape[0], 5, buf.ctypes.data, need, ne, got.ctypes.data) \
        == _lib.ERR_ARG
    bad = boxes.copy()
    bad[3, 1] = np.nan
    assert lib.bo_ehvi_tables(bad.ctypes.data, bad.shape[0], 2, buf.ctypes.data, need, ne, got.ctypes.data) \
        == _lib.ERR_ARG


def test_admission_rule_mirror():
    from bayesopt_smart_amd import _lib
    lib = _lib.load()
    for s in list(range(0, 400)) + [1 << 20, 1 << 40]:
        assert lib.bo_ehvi_table_threads(s) == R.table_threads(s), s
    assert [R.table_threads(s) for s in (80, 81, 160, 161, 320, 321)] == [256, 128, 128, 64, 64, 0]
    assert lib.bo_ehvi_table_threads(-1) == 0


def test_scan_argument_checks_return_before_the_device():
    """Every call here returns from the argument checks, before any HIP call."""
    from bayesopt_smart_amd import _lib
    lib = _lib.load()
    ne = (ctypes.c_int32 * 2)(200, 200)
    p = 4096                                                # never dereferenced
    f = lib.bo_expected_hypervolume_improvement
    assert f(None, p, p, 8, 8, 2, p, 1, p, ne, p, 0, None) == _lib.ERR_ARG
    assert f(p, p, p, 7, 8, 2, p, 1, p, ne, p, 0, None) == _lib.ERR_ARG          # ld < n
    assert f(p, p, p, 8, 8, 5, p, 1, p, ne, p, 0, None) == _lib.ERR_ARG          # n_obj > 4
    assert f(p, p, p, 8, 8, 2, p, 1, p, ne, p, 3, None) == _lib.ERR_ARG          # form
    assert f(p, p, p, 8, 8, 2, None, 1, p, ne, p, 1, None) == _lib.ERR_ARG       # direct without boxes
    assert f(p, p, p, 8, 8, 2, p, 1, None, ne, p, 2, None) == _lib.ERR_ARG       # table without edges
    assert f(p, p, p, 8, 8, 2, p, 1, p, ne, p, 2, None) == _lib.ERR_UNSUPPORTED  # 400 edges: no table fits
    assert f(p, p, p, 8, 0, 2, p, 1, p, ne, p, 0, None) == _lib.OK               # nothing to do


def test_limits_and_errors():
    from bayesopt_smart_amd.bayesian_optimization import _check_limits
    with pytest.raises(ValueError, match="4 objectives"):
        _check_limits(5, 2, 64, 3, acquisition="ehvi")
    _check_limits(4, 2, 64, 3, acquisition="ehvi")
    with pytest.raises(ValueError):
        _check_limits(2, 2, 64, 3, acquisition="ehvi", batch_strategy="bucb")
    from bayesopt_smart_amd.acquisition import expected_hypervolume_improvement
    with pytest.raises(ValueError, match="form"):
        expected_hypervolume_improvement(np.zeros((2, 4)), np.ones((2, 4)), np.zeros((0, 2)), np.zeros(2),
                                         form="fast")

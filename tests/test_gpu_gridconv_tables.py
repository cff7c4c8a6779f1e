"""GPU tests of the grid-convolution path's exp tables (bo_gridconv.hip conv_tables): the list kernel builds
tabE, tabB, tabH and the two bands once per call and distinct length scale in the workspace, and the
accumulate kernel and the contraction copy them into LDS.

Three objectives with length scales (6, 6, 2.5): two objectives share one set of tables, the third has its
own, and at C > 64 the bands are not full.  Every case runs in mode="auto-conv"; mu, var and acq are compared
with the CPU reference (tests/fullref.py) under tests/parity.py's rule, as tests/test_gpu_gridconv.py does.
One case has a length scale so large that no table entry is flushed (hq = LT - 1, hm = C - 1) and one so
small that only t = 0 survives in tabH (hm = 0)."""

import numpy as np
import pytest

from oracle import oracle_np as O
import fullref
import gridconv_model as G
from parity import check_predict

pytestmark = pytest.mark.gpu

ALL = ("mu", "var", "std_mu", "std_var", "ucb", "acq")
TAB_FLUSH = 2.0 ** -128          # bo_gridconv.hip: kTabFlush
LS = (6.0, 6.0, 2.5)

# (shape, rows x columns of the point lattice, its spacings, jitter of +-1 per coordinate, length scales): the
# points are at least 5 apart, so that cond(K + 1e-6 I) stays below 1e6 (the parity rule's domain) at these
# length scales, and several share a column
CASES = {
    "r40": ((40, 80), (6, 10), (7, 8), True, LS),              # R no multiple of 16, C no multiple of 64: N = 60
    "r33": ((33, 200), (4, 24), (8, 8), True, LS),             # N = 96
    "wide": ((40, 80), (6, 10), (7, 8), False, (9.0, 9.0, 9.0)),       # nothing flushed
    "narrow": ((40, 80), (6, 10), (7, 8), True, (0.07, 0.07, 0.07)),   # H(t) flushed for every t != 0
}


@pytest.fixture(scope="module")
def bo():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import bayesopt_smart_amd as bo
    bo._lib.load()
    return bo


_PROBLEMS = {}


def _problem(name):
    """(shape, problem, CPU reference), computed once per case; the objectives as gridconv_model.lattice_problem
    draws them."""
    if name not in _PROBLEMS:
        shape, (nr, nc), (dr, dc), jitter, ls = CASES[name]
        rng = np.random.default_rng(71)
        rel = np.array([(2 + dr * a, 3 + dc * b) for a in range(nr) for b in range(nc)], dtype=np.int64)
        if jitter:
            rel = rel + rng.integers(-1, 2, size=rel.shape)
        rel = rel[rng.permutation(rel.shape[0])]
        n, n_obj = rel.shape[0], len(ls)
        assert rel.min() >= 0 and rel[:, 0].max() < shape[0] and rel[:, 1].max() < shape[1]
        assert np.bincount(rel[:, 1]).max() > 1
        x = rel.astype(np.float64)
        y = rng.normal(size=(n, n_obj)) * 30 + 5
        pm, pv = y.mean(0), y.var(0)
        ls = np.asarray(ls, dtype=np.float64)
        betas = rng.uniform(0.5, 2.5, size=n_obj)
        km = np.zeros((n_obj, n, n))
        O.update_k(km, x, 0, n, pv, ls)
        assert max(np.linalg.cond(km[o] + 1e-6 * np.eye(n)) for o in range(n_obj)) < 1e6
        d = dict(x=x, y=y, pm=pm, pv=pv, ls=ls, betas=betas, Kinv=O.invert_k(n, km))
        assert G.conv_planned(shape, n, n_obj, mode="auto-conv")
        ref = fullref.cpu_full(("gridconv-tables", name), x, y, G.grid_points(shape, (0, 0)), d["Kinv"], pm, pv, ls,
                               betas)
        _PROBLEMS[name] = (shape, d, ref)
    return _PROBLEMS[name]


def _bands(shape, ls):
    """(hq, hm) by the kernel's comparison: the largest |t| whose table entry is not below kTabFlush."""
    C = shape[1]
    LT = -(-(2 * C - 1) // 16) * 16
    nhl = -0.5 / (ls * ls)
    tq, tm = np.arange(LT, dtype=np.float64), np.arange(C, dtype=np.float64)
    return (int(np.flatnonzero(~(np.exp(0.5 * nhl * (tq * tq)) < TAB_FLUSH)).max()),
            int(np.flatnonzero(~(np.exp(nhl * (tm * tm)) < TAB_FLUSH)).max()))


def _cands(bo, shape):
    return bo.predict.CandidateSet.grid([(0, shape[0]), (0, shape[1])])


def _prepared(bo, d, shape, q, mode, offset=0, count=None):
    return bo.predict.predict_acquire(d["x"], d["y"], d["Kinv"], _cands(bo, shape), d["pm"], d["pv"], d["ls"],
                                      d["betas"], outputs=ALL, topq=q, offset=offset, count=count, mode=mode,
                                      prepare=True)


def _outputs(res):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items() if not k.startswith("_")}


def _call(bo, d, shape, q=3, mode="auto-conv", offset=0, count=None):
    return _outputs(_prepared(bo, d, shape, q, mode, offset, count)())


def _bit_equal(a, b):
    assert set(a) == set(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_the_cases_are_what_they_claim():
    """Two objectives share a length scale and one does not; the bands of the two shapes are not full; the
    wide case flushes nothing and the narrow one keeps H(0) alone."""
    assert LS[0] == LS[1] != LS[2]
    for name in ("r40", "r33"):
        shape = CASES[name][0]
        LT = -(-(2 * shape[1] - 1) // 16) * 16
        bands = [_bands(shape, ls) for ls in LS]
        assert all(0 < hq < LT - 1 and 0 < hm for hq, hm in bands)
        # (at C = 80 H(79) at length scale 6 is not flushed: there only the third objective's mean band is cut)
        assert bands[2][1] < shape[1] - 1 and (bands[0][1] < shape[1] - 1 or shape[1] == 80)
    shape = CASES["wide"][0]
    assert _bands(shape, CASES["wide"][4][0]) == (-(-(2 * shape[1] - 1) // 16) * 16 - 1, shape[1] - 1)
    hq, hm = _bands(CASES["narrow"][0], CASES["narrow"][4][0])
    assert hm == 0 and hq >= 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_parity_and_band_equals_full(bo, name):
    shape, d, ref = _problem(name)
    out = _call(bo, d, shape)
    check_predict({k: out[k] for k in ("mu", "var", "acq")}, ref, d["pv"])
    _bit_equal(out, _call(bo, d, shape, mode="auto-conv-full"))


@pytest.mark.parametrize("name", ["r40", "r33"])
def test_two_shards_equal_the_whole_call(bo, name):
    shape, d, _ = _problem(name)
    total = shape[0] * shape[1]
    cut = 11 * shape[1] + 7                       # the second shard starts inside a grid row
    whole = _call(bo, d, shape, q=5)
    parts = [_call(bo, d, shape, q=5, offset=0, count=cut), _call(bo, d, shape, q=5, offset=cut, count=total - cut)]
    for k in ALL:
        np.testing.assert_array_equal(np.concatenate([p[k] for p in parts], axis=-1), whole[k], err_msg=k)
    v, i = bo.predict.merge_topq(np.concatenate([p["top_val"] for p in parts]),
                                 np.concatenate([p["top_idx"] for p in parts]), 5)
    np.testing.assert_array_equal(i, whole["top_idx"])
    np.testing.assert_array_equal(v, whole["top_val"])


@pytest.mark.parametrize("name", ["r40", "r33"])
def test_second_call_and_replay_over_a_workspace_of_ones(bo, name):
    """The band words are zeroed and raised, and every table entry written, inside the sequence itself."""
    import torch
    shape, d, _ = _problem(name)
    call = _prepared(bo, d, shape, 3, "auto-conv")
    nbytes = int(bo._lib.load().bo_predict_workspace_size(call._desc))
    buf = torch.empty(nbytes, dtype=torch.uint8, device=call._ws.device)
    assert buf.data_ptr() % 256 == 0
    call._ws, call._ws_ptr, call._ws_n = buf, buf.data_ptr(), nbytes

    def clear():
        for t in call.res.values():
            if isinstance(t, torch.Tensor):
                t.zero_()
        buf.fill_(0xFF)

    first = _call(bo, d, shape)
    clear()
    _bit_equal(_outputs(call()), first)
    replay = call.graphed()
    clear()
    _bit_equal(_outputs(replay()), first)

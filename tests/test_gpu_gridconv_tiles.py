"""GPU tests of the contraction's wave-tile widths (bo_gridconv.hip, conv_contract_kernel<NB>): the outputs
and the selection do not depend on the tile (BO_CONV_TILE = 1, 2, 4: 16, 32 and 64 columns) nor on the
k-blocks that a narrower band skips ("auto-conv-full" runs them all), bit for bit, and agree with the
chunk-major kernel ("auto-noconv") under the project's tolerance rule."""

import contextlib
import os

import numpy as np
import pytest

from oracle import oracle_np as O
from parity import check_predict

pytestmark = pytest.mark.gpu

ALL = ("mu", "var", "std_mu", "std_var", "ucb", "acq")
TILES = ("1", "2", "4")
FLUSH = 2.0 ** -128            # bo_gridconv.hip: kTabFlush


@pytest.fixture(scope="module")
def bo():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import bayesopt_smart_amd as bo
    bo._lib.load()
    return bo


@contextlib.contextmanager
def _tile(nb):
    """BO_CONV_TILE for the calls planned inside (the plan reads it per call)."""
    old = os.environ.get("BO_CONV_TILE")
    if nb is None:
        os.environ.pop("BO_CONV_TILE", None)
    else:
        os.environ["BO_CONV_TILE"] = nb
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("BO_CONV_TILE", None)
        else:
            os.environ["BO_CONV_TILE"] = old


def _cands(bo, shape):
    return bo.predict.CandidateSet.grid([(0, shape[0]), (0, shape[1])])


def _call(bo, d, cands, q, outputs=ALL, mode="auto-conv", offset=0, count=None):
    import torch
    res = bo.predict.predict_acquire(d["x"], d["y"], d["Kinv"], cands, d["pm"], d["pv"], d["ls"], d["betas"],
                                     outputs=outputs, topq=q, offset=offset, count=count, mode=mode)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items() if not k.startswith("_")}


def _finish(x, y, ls, betas, pm=None, pv=None):
    n, n_obj = y.shape
    pm = y.mean(0) if pm is None else pm
    pv = y.var(0) if pv is None else pv
    ls = np.asarray(ls, dtype=np.float64)
    km = np.zeros((n_obj, n, n))
    O.update_k(km, x, 0, n, pv, ls)
    assert max(np.linalg.cond(km[o] + 1e-6 * np.eye(n)) for o in range(n_obj)) < 1e6
    return dict(x=x, y=y, pm=pm, pv=pv, ls=ls, betas=np.asarray(betas, dtype=np.float64), Kinv=O.invert_k(n, km))


def _two_sided(n_obj, ls, seed):
    """40 x 200, N = 24: the points in the columns 0 .. 40 and 150 .. 199 (columns 0 and 199 among them),
    none between."""
    rng = np.random.default_rng(seed)
    pts = {(3, 0), (31, 0), (17, 199), (38, 199)}
    while len(pts) < 24:
        c = int(rng.integers(0, 41)) if rng.random() < 0.5 else int(rng.integers(150, 200))
        pts.add((int(rng.integers(40)), c))
    x = np.array(sorted(pts), dtype=np.float64)[rng.permutation(24)]
    y = rng.normal(size=(24, n_obj)) * 30 + 5
    return _finish(x, y, ls, rng.uniform(0.5, 2.5, size=n_obj))


SHAPE = (40, 200)
_CACHE = {}


def _runs(bo, name, make, shape, q, outputs=ALL, offset=0, count=None):
    """The case's results, computed once: the three widths, every k-block, and the chunk-major kernel."""
    if name not in _CACHE:
        d = make()
        cands = _cands(bo, shape)
        kw = dict(outputs=outputs, offset=offset, count=count)
        runs = {}
        for nb in TILES:
            with _tile(nb):
                runs[nb] = _call(bo, d, cands, q, **kw)
        with _tile(None):
            runs["full"] = _call(bo, d, cands, q, mode="auto-conv-full", **kw)
            runs["noconv"] = _call(bo, d, cands, q, mode="auto-noconv", **kw)
        _CACHE[name] = (d, cands, runs)
    return _CACHE[name]


def _check(d, runs, outputs=ALL, differs=True):
    first = runs[TILES[0]]
    assert set(outputs) <= set(first) and {"top_idx", "top_val"} <= set(first)
    for other in TILES[1:] + ("full",):
        assert set(runs[other]) == set(first)
        for k in first:
            assert np.array_equal(runs[other][k], first[k]), (other, k)
    # the grid-convolution kernels did run (the regrouped variance differs in its last bits; not asserted where
    # a variance is one product)
    if differs:
        assert (first["var"] != runs["noconv"]["var"]).any()
    check_predict({k: first[k] for k in outputs}, {k: runs["noconv"][k] for k in outputs}, d["pv"])


def _library_order(acq, excl, q):
    a = np.where(excl, -np.inf, acq)
    return np.lexsort((np.arange(a.size), -a))[:q]


def _excl_mask(d, shape, offset=0, count=None):
    lin = (d["x"][:, 0] * shape[1] + d["x"][:, 1]).astype(np.int64)
    m = np.zeros(shape[0] * shape[1], dtype=bool)
    m[lin] = True
    return m[offset:(None if count is None else offset + count)]


def test_ragged_grid_narrow_bands(bo):
    """R no multiple of 16, C no multiple of 32 or 64 (the tiles from column 208 on are padding alone, the
    one at 192 partly), points in the first and the last column, and a length scale whose bands are well
    below C / 2: the 16-column tiles skip k-blocks that the 64-column tiles run, and the tile at column 80
    has no point within its mean band."""
    d, cands, runs = _runs(bo, "ragged", lambda: _two_sided(2, [2.5, 2.5], 11), SHAPE, 8)
    R, C = SHAPE
    assert R % 16 and C % 32 and C % 64 and -(-C // 64) * 64 - C >= 48
    cols = d["x"][:, 1]
    assert (cols == 0).any() and (cols == C - 1).any()
    t = np.arange(C)
    hm = int(t[np.exp(-t.astype(np.float64) ** 2 / (2 * 2.5 ** 2)) >= FLUSH].max())
    hq = int(np.arange(2 * C)[np.exp(-np.arange(2 * C, dtype=np.float64) ** 2 / (4 * 2.5 ** 2)) >= FLUSH].max())
    assert hq < C // 2
    assert not ((cols >= 80 - hm) & (cols <= 95 + hm)).any(), "the 16-column tile at 80 has points in its band"
    assert ((cols >= 64 - hm) & (cols <= 127 + hm)).any()
    _check(d, runs)
    want = _library_order(runs["1"]["acq"], _excl_mask(d, SHAPE), 8)
    np.testing.assert_array_equal(runs["1"]["top_idx"], want)


def test_ragged_grid_as_a_shard(bo):
    """The same grid from an odd offset inside a row to the middle of another: the first and the last tile's
    candidate bounds, and outputs that start at an odd element."""
    offset, count = 3 * 200 + 77, 4321
    assert offset % 2 == 1 and offset % 200 and (offset + count) % 200
    d, cands, runs = _runs(bo, "shard", lambda: _two_sided(2, [2.5, 2.5], 11), SHAPE, 8, offset=offset, count=count)
    _check(d, runs)
    whole = _runs(bo, "ragged", lambda: _two_sided(2, [2.5, 2.5], 11), SHAPE, 8)[2]["1"]
    for k in ALL:
        assert np.array_equal(runs["1"][k], whole[k][..., offset:offset + count]), k
    want = offset + _library_order(runs["1"]["acq"], _excl_mask(d, SHAPE, offset, count), 8)
    np.testing.assert_array_equal(runs["1"]["top_idx"], want)


def test_three_length_scales(bo):
    """Three objectives, three length scales: the tables are rebuilt per objective inside the tile loop, and
    each objective has bands of its own."""
    d, cands, runs = _runs(bo, "three", lambda: _two_sided(3, [1.8, 2.5, 3.4], 12), SHAPE, 8)
    assert len(set(d["ls"])) == 3
    _check(d, runs)


def _symmetric():
    """1024 x 1024, eight isolated points, symmetric about the grid centre in place and value, beta = 0: the
    acquisition peaks at the points (evaluated: excluded), and around a point and its mirror image the
    same values stand in rings -- exact ties, since each is one product of the same factors (every other
    term is an exact zero)."""
    side = 1024
    half = np.array([(16, 64), (300, 500), (500, 100), (200, 800)], dtype=np.float64)
    x = np.concatenate([half, side - 1 - half])
    y0 = np.array([100.0, 60.0, -50.0, 10.0])
    y = np.stack([np.tile(y0, 2), 0.5 * np.tile(y0, 2)], axis=1)
    return _finish(x, y, [2.5, 2.5], [0.0, 0.0])


@pytest.mark.parametrize("q", [5, 48])
def test_selection_ties_across_waves_and_workgroups(bo, q):
    side = 1024
    outs = ("mu", "var", "ucb", "acq")
    d, cands, runs = _runs(bo, ("sym", q), _symmetric, (side, side), q, outputs=outs)
    _check(d, runs, outs, differs=False)
    out = runs["1"]
    acq, excl = out["acq"], _excl_mask(d, (side, side))
    raw = np.lexsort((np.arange(acq.size), -acq))[:2]
    assert excl[raw].all(), "no evaluated point at the top"
    want = _library_order(acq, excl, q)
    np.testing.assert_array_equal(out["top_idx"], want)
    np.testing.assert_array_equal(out["top_val"], acq[want])
    # the best value stands at the four neighbours of (16, 64) and of its image (1007, 959): in four wave
    # tiles each for every width up to 32 columns, and in workgroups at both ends of the grid
    best = np.flatnonzero(np.where(excl, -np.inf, acq) == acq[want[0]])
    assert set(best) == {15 * side + 64, 16 * side + 63, 16 * side + 65, 17 * side + 64,
                         1006 * side + 959, 1007 * side + 958, 1007 * side + 960, 1008 * side + 959}
    assert set(want[:min(q, 8)]) <= set(best)


def test_fewer_tiles_than_waves(bo):
    """16 x 16, N = 2: one 64-column tile (four of 16 columns, three of them padding); the waves without a
    tile still take part in the workgroup's list merge."""
    def make():
        x = np.array([(4.0, 5.0), (11.0, 9.0)])
        y = np.array([[3.0, -1.0], [-2.0, 4.0]])
        return _finish(x, y, [2.0, 2.0], [1.0, 1.5], pm=np.array([0.5, 1.0]), pv=np.array([6.0, 6.0]))
    d, cands, runs = _runs(bo, "tiny", make, (16, 16), 48)
    _check(d, runs, differs=False)
    want = _library_order(runs["1"]["acq"], _excl_mask(d, (16, 16)), 48)
    np.testing.assert_array_equal(runs["1"]["top_idx"], want)


@pytest.mark.parametrize("nb", TILES)
def test_graph_replays_over_a_garbage_workspace(bo, nb):
    """The symmetric case captured as a HIP graph and replayed twice, the workspace (the partial lists among
    it) filled with garbage before each replay: bit equal to the direct call."""
    import torch
    outs = ("mu", "var", "ucb", "acq")
    d, cands, runs = _runs(bo, ("sym", 5), _symmetric, (1024, 1024), 5, outputs=outs)
    with _tile(nb):
        prepared = bo.predict.predict_acquire(d["x"], d["y"], d["Kinv"], cands, d["pm"], d["pv"], d["ls"], d["betas"],
                                              outputs=outs, topq=5, mode="auto-conv", prepare=True)
        replay = prepared.graphed()
    for _ in range(2):
        for t in prepared.res.values():
            if isinstance(t, torch.Tensor):
                t.zero_()
        prepared._ws.fill_(0x7F)
        res = replay()
        torch.cuda.synchronize()
        for k in runs[nb]:
            assert np.array_equal(res[k].cpu().numpy(), runs[nb][k]), k

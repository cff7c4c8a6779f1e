"""GPU tests of the contraction's exclusion of evaluated points (bo_gridconv.hip): when a call excludes its own
training points, each wave marks those of its tile from the LDS copy of their coordinates before the selection
rounds; with an exclusion set of the caller's the rounds probe the prep launch's hash set as before.

The problem is test_gpu_gridconv.py::test_topq_exclusion_at_the_top's (beta = 0 and a short length scale: the
acquisition peaks AT the best training points, so evaluated points lead the order), with the best training
points placed where the marking can go wrong: the four corners of a wave tile for every tile width
(BO_CONV_TILE = 1, 2, 4: 16, 32 and 64 columns), two in one tile, and the last column of the grid -- on the
64 x 120 grid that is a partly padded column tile (64 x 128 has none).  The selection is judged against the CPU
reference's acquisition array and its `select` by bench.selection_check's tie-aware rule, and against the same
call's chunk-major result (mode "auto-noconv")."""

import numpy as np
import pytest

from oracle import cpu_ref
from oracle import oracle_np as O
import fullref
import gridconv_model as G
from test_gpu_gridconv_tiles import _tile

pytestmark = pytest.mark.gpu

N = 40
SHAPES = ((64, 128), (64, 120))
I0, J0 = 16, 64          # a wave tile's first row and column, for every tile width
assert SHAPES[1][1] % 16 != 0 and -(-SHAPES[1][1] // 64) == -(-SHAPES[0][1] // 64)


@pytest.fixture(scope="module")
def bo():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import bayesopt_smart_amd as bo
    bo._lib.load()
    return bo


def _special(C):
    """The training points that lead the acquisition's order, best first."""
    corners = [(r, c) for c in (J0, J0 + 15, J0 + 31, min(J0 + 63, C - 1)) for r in (I0, I0 + 15)]
    # and two inside one tile of every width (far enough apart that the mean does not overshoot between them)
    return corners + [(34, 2), (45, 13)]


_PROBLEMS = {}


def _problem(shape):
    """(problem, grid points, CPU reference acquisition), once per shape."""
    if shape not in _PROBLEMS:
        R, C = shape
        rng = np.random.default_rng(25)
        top = _special(C)
        have, pts = set(top), list(top)
        while len(pts) < N:
            p = (int(rng.integers(R)), int(rng.integers(C)))
            # (no other training point near a leading one: its neighbours are the best candidates left)
            if p not in have and all(abs(p[0] - t[0]) > 8 or abs(p[1] - t[1]) > 8 for t in top):
                have.add(p)
                pts.append(p)
        x = np.array(pts, dtype=np.float64)
        y = rng.normal(size=(N, 2))
        y[:len(top), 0] = 1000.0 - 2.0 * np.arange(len(top))
        y[:len(top), 1] = 50.0 - 0.1 * np.arange(len(top))
        pm, pv = y.mean(0), y.var(0)
        ls, betas = np.array([3.0, 3.0]), np.zeros(2)
        km = np.zeros((2, N, N))
        O.update_k(km, x, 0, N, pv, ls)
        d = dict(x=x, y=y, pm=pm, pv=pv, ls=ls, betas=betas, Kinv=O.invert_k(N, km))
        assert G.conv_planned(shape, N, 2, mode="auto-conv")
        grid = G.grid_points(shape, (0, 0))
        acq = fullref.cpu_full(("gridconv-exclusion", shape), x, y, grid, d["Kinv"], pm, pv, ls, betas)["acq"]
        # every one of the leading training points comes before every candidate that is none
        lin = np.array([r * C + c for r, c in top])
        rest = np.ones(R * C, dtype=bool)
        rest[(x[:, 0] * C + x[:, 1]).astype(np.int64)] = False
        assert acq[lin].min() > acq[rest].max(), "an evaluated point does not lead the order"
        _PROBLEMS[shape] = (d, grid, acq)
    return _PROBLEMS[shape]


def _exclusion(d, shape, explicit):
    """(excl_points argument, mask over the grid).  The explicit set drops two training points (the best one
    among them) and adds two grid points that are none: it differs from the training set both ways."""
    C = shape[1]
    pts = d["x"]
    if explicit:
        pts = np.concatenate([d["x"][1:9], d["x"][10:], [[I0, J0 + 1], [I0 + 1, J0]]])
        assert pts.shape[0] == N
    mask = np.zeros(shape[0] * C, dtype=bool)
    mask[(pts[:, 0] * C + pts[:, 1]).astype(np.int64)] = True
    return (pts.copy() if explicit else None), mask


def _select(bo, d, shape, q, excl, mode):
    import torch
    cands = bo.predict.CandidateSet.grid([(0, shape[0]), (0, shape[1])])
    res = bo.predict.predict_acquire(d["x"], d["y"], d["Kinv"], cands, d["pm"], d["pv"], d["ls"], d["betas"],
                                     outputs=("acq",), topq=q, excl_points=excl, mode=mode)
    torch.cuda.synchronize()
    return res["top_idx"].cpu().numpy(), res["acq"].cpu().numpy()


@pytest.mark.parametrize("explicit", [False, True], ids=["train", "explicit"])
@pytest.mark.parametrize("nb", ["1", "2", "4"])
@pytest.mark.parametrize("shape", SHAPES, ids=["c128", "c120"])
def test_selection_steps_over_evaluated_points(bo, shape, nb, explicit):
    import bench
    d, grid, cpu_acq = _problem(shape)
    excl, mask = _exclusion(d, shape, explicit)
    for q in range(1, 6):
        ref_sel = cpu_ref.select(cpu_acq, grid.astype(np.float64), d["x"] if excl is None else excl, q)
        assert bench.selection_check(ref_sel, cpu_acq, mask, q)
        with _tile(nb):
            got, acq = _select(bo, d, shape, q, excl, "auto-conv")
        assert not mask[got].any(), "selected an evaluated point"
        assert bench.selection_check(got, cpu_acq, mask, q), (q, got, ref_sel)
        # exactly the order of the call's own acquisition array
        want = np.lexsort((np.arange(acq.size), -np.where(mask, -np.inf, acq)))[:q]
        np.testing.assert_array_equal(got, want)
        old, old_acq = _select(bo, d, shape, q, excl, "auto-noconv")
        assert bench.selection_check(got, old_acq, mask, q), (q, got, old)
        assert bench.selection_check(old, acq, mask, q), (q, got, old)

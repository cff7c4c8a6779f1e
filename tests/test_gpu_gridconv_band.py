"""GPU tests of what the grid-convolution path leaves out (bo_gridconv.hip): the training pairs
whose weight is negligible for every objective (conv_list_kernel compacts the list, conv_acc_kernel
runs the kept part) and the k-blocks of the two contractions whose table entries were flushed to zero
for a whole wave tile (conv_contract_kernel: the tau outside the tile's band in the variance GEMM,
the training points of far columns in the mean GEMM, whose rows are in column order).

The cases have more than 64 columns (with C <= 64 the band 126 + 2h covers every tau) and length
scales short enough that pairs are dropped and the band is narrower than the tau range; both are
asserted here from the inputs, with the kernels' own criteria.  "auto-conv-full" runs every k-block
over the same table and the same list: the band must equal it bit for bit."""

import numpy as np
import pytest

from oracle import oracle_np as O
from parity import check_predict, check_topq
import gridconv_model as G

pytestmark = pytest.mark.gpu

ALL = ("mu", "var", "std_mu", "std_var", "ucb", "acq")
PAIR_DROP = 2.0 ** -100         # bo_gridconv.hip: kPairDrop
TAB_FLUSH = 2.0 ** -128         # kTabFlush

# name: shape, lo, n, n_obj, seed, ls
CASES = {
    "A": ((40, 200), (0, 0), 60, 2, 11, (1.5, 3.0)),
    "B": ((70, 300), (-5, 11), 150, 3, 12, (2.0, 2.0, 5.0)),     # tables kept for one objective, rebuilt for the next
    "C": ((96, 260), (3, -2), 90, 2, 13, (2.5, 4.0)),
}
LATTICE = ((37, 50), (10 ** 6, -7), 40, 2, 5, None)              # test_gpu_gridconv.py's case: both bands full


@pytest.fixture(scope="module")
def bo():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import bayesopt_smart_amd as bo
    bo._lib.load()
    return bo


def _cands(bo, shape, lo):
    return bo.predict.CandidateSet.grid([(lo[0], lo[0] + shape[0]), (lo[1], lo[1] + shape[1])])


def _call(bo, d, cands, q, outputs=ALL, mode="auto-conv", offset=0, count=None):
    import torch
    res = bo.predict.predict_acquire(d["x"], d["y"], d["Kinv"], cands, d["pm"], d["pv"], d["ls"], d["betas"],
                                     outputs=outputs, topq=q, offset=offset, count=count, mode=mode)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items() if not k.startswith("_")}


def _excluded(pts, x):
    xs = {tuple(r) for r in np.asarray(x, dtype=np.float64)}
    return np.array([tuple(np.asarray(c, dtype=np.float64)) in xs for c in pts])


_PROBLEMS = {}


def _problem(case):
    """(shape, lo, problem, grid points, oracle outputs), computed once per case."""
    if case not in _PROBLEMS:
        shape, lo, n, n_obj, seed, ls = case
        d = G.lattice_problem(shape, lo, n, n_obj, seed, ls=ls)
        pts = G.grid_points(shape, lo)
        ref = O.predict_acquire(d["x"], d["y"], pts, d["pm"], d["pv"], d["ls"], d["betas"], kinv=d["Kinv"])
        _PROBLEMS[case] = (shape, lo, d, pts, ref)
    return _PROBLEMS[case]


def _pairs_kept(d):
    """The list kernel's criterion on every pair n <= m: kept when |w_o| >= 2^-100 pv_o for some
    objective.  Returns (n, m, kept) over the upper triangle."""
    rel, kinv, pv, ls = d["rel"], d["Kinv"], d["pv"], d["ls"]
    iu = np.triu_indices(rel.shape[0])
    d2 = ((rel[iu[0]] - rel[iu[1]]) ** 2).sum(1).astype(np.float64)
    keep = np.zeros(iu[0].size, dtype=bool)
    for o in range(len(pv)):
        sym = np.where(iu[0] == iu[1], kinv[o][iu], kinv[o][iu] + kinv[o].T[iu])
        w = sym * (pv[o] * pv[o]) * np.exp(-d2 / (4.0 * ls[o] ** 2))
        keep |= ~(np.abs(w) < PAIR_DROP * pv[o])
    return iu[0], iu[1], keep


def _band(ls, extent):
    """Largest |t| < extent with E(t) = exp(-t^2 / 4 l^2) not flushed."""
    t = np.arange(extent, dtype=np.float64)
    return int(np.flatnonzero(~(np.exp(-t * t / (4.0 * ls * ls)) < TAB_FLUSH)).max())


def _assert_exercised(case):
    """The case drops pairs, keeps pairs, has a non-empty tau that keeps nothing, and bands that leave
    out k-blocks of a 64-column tile in both GEMMs."""
    shape, lo, d, _, _ = _problem(case)
    C = shape[1]
    n_, m_, keep = _pairs_kept(d)
    assert keep.any() and not keep.all()
    tau = d["rel"][n_, 1] + d["rel"][m_, 1]
    total, kept = np.bincount(tau, minlength=2 * C - 1), np.bincount(tau[keep], minlength=2 * C - 1)
    assert ((total > 0) & (kept == 0)).any(), "no tau whose pairs are all dropped"
    LT = -(-(2 * C - 1) // 16) * 16
    assert all(126 + 2 * _band(l, LT) < 2 * C - 1 - 32 for l in d["ls"]), "the variance band is full"
    # the mean GEMM's rows are in column order: a tile runs the k-blocks of the points within h_H columns
    cstart = np.searchsorted(np.sort(d["rel"][:, 1]), np.arange(C + 1))
    n_kb = -(-d["rel"].shape[0] // 16)
    for l in d["ls"]:
        t = np.arange(2 * C, dtype=np.float64)
        hm = int(np.flatnonzero(~(np.exp(-t * t / (2.0 * l * l)) < TAB_FLUSH)).max())
        run = [-(-cstart[min(C, j0 + 64 + hm)] // 16) - cstart[max(0, j0 - hm)] // 16 for j0 in range(0, C, 64)]
        assert min(run) < n_kb, "the mean band is full"


def _check_parity(bo, shape, lo, d, pts, ref, q):
    assert G.conv_planned(shape, d["x"].shape[0], len(d["pm"]), mode="auto-conv")
    cands = _cands(bo, shape, lo)
    out = _call(bo, d, cands, q)
    old = _call(bo, d, cands, q, outputs=("var",), mode="auto-noconv")
    assert (out["var"] != old["var"]).any(), "auto-conv ran the chunk-major kernel"
    check_predict(out, ref, d["pv"])
    excl = _excluded(pts, d["x"])
    check_topq(out["top_idx"], ref["acq"], excl, q)
    # the selection is exactly the order of the call's own acquisition array
    a = np.where(excl, -np.inf, out["acq"])
    want = np.lexsort((np.arange(a.size), -a))[:q]
    np.testing.assert_array_equal(out["top_idx"], want)
    np.testing.assert_array_equal(out["top_val"], out["acq"][want])


@pytest.mark.parametrize("q", [3, 16])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_parity(bo, name, q):
    case = CASES[name]
    _assert_exercised(case)
    shape, lo, d, pts, ref = _problem(case)
    _check_parity(bo, shape, lo, d, pts, ref, q)


@pytest.mark.parametrize("name", ["A", "B", "C", "LATTICE"])
def test_band_equals_full_range(bo, name):
    """Every output and the selection of "auto-conv" equal "auto-conv-full" bit for bit: a skipped
    k-block multiplies finite T by exact zeros."""
    shape, lo, d, _, _ = _problem(CASES.get(name, LATTICE))
    cands = _cands(bo, shape, lo)
    band = _call(bo, d, cands, 16)
    full = _call(bo, d, cands, 16, mode="auto-conv-full")
    assert set(band) == set(full) == set(ALL) | {"top_idx", "top_val"}
    for k in band:
        np.testing.assert_array_equal(band[k], full[k], err_msg=k)


def test_shards_equal_the_whole_call(bo):
    """C in four shards that start and end mid-row; the cut at row 30 lies inside a 16-row tile of the
    whole call.  A tile's outputs do not depend on which k-blocks were skipped or on the shard's rows."""
    shape, lo, d, _, _ = _problem(CASES["C"])
    C = shape[1]
    cands = _cands(bo, shape, lo)
    whole = _call(bo, d, cands, 16)
    bounds = [3 * C + 5, 30 * C + 7, 53 * C + 100, 77 * C + 33, shape[0] * C - 9]
    assert all(b % C for b in bounds) and (bounds[1] // C) % 16
    vals, idxs = [], []
    for a, b in zip(bounds[:-1], bounds[1:]):
        r = _call(bo, d, cands, 16, offset=a, count=b - a)
        for k in ALL:
            np.testing.assert_array_equal(r[k], whole[k][..., a:b], err_msg=f"{k} of shard [{a}, {b})")
        vals.append(r["top_val"])
        idxs.append(r["top_idx"])
    span = _call(bo, d, cands, 16, outputs=("acq",), offset=bounds[0], count=bounds[-1] - bounds[0])
    v, i = bo.predict.merge_topq(np.concatenate(vals), np.concatenate(idxs), 16)
    np.testing.assert_array_equal(i, span["top_idx"])
    np.testing.assert_array_equal(v, span["top_val"])


def test_graph_replays_over_a_garbage_workspace(bo):
    """A from one captured graph whose workspace is filled with garbage before every replay: the kept
    counts, the compacted list and the T rows of the tau that keep nothing are all rewritten by the
    captured sequence."""
    import torch
    shape, lo, d, _, _ = _problem(CASES["A"])
    cands = _cands(bo, shape, lo)
    runs = [_call(bo, d, cands, 16)]
    prepared = bo.predict.predict_acquire(d["x"], d["y"], d["Kinv"], cands, d["pm"], d["pv"], d["ls"], d["betas"],
                                          outputs=ALL, topq=16, mode="auto-conv", prepare=True)
    replay = prepared.graphed()
    for _ in range(3):
        for t in prepared.res.values():
            if isinstance(t, torch.Tensor):
                t.zero_()
        prepared._ws.fill_(0x7F)             # kept counts far past the lists, T entries of 1e306
        res = replay()
        torch.cuda.synchronize()
        runs.append({k: res[k].cpu().numpy() for k in runs[0]})
    assert len(runs) == 4
    for r in runs[1:]:
        for k in runs[0]:
            assert np.array_equal(r[k], runs[0][k]), k


def test_only_the_diagonal_is_kept(bo):
    """8 points 28 columns apart on (16, 200), l = 1.5: every pair n < m is dropped, every tau holds at
    most its diagonal pair.  (8 points cannot lie 60 columns apart in 200 columns; 28 is the widest
    even spacing that fits, and the list kernel's criterion is asserted on the inputs below.)"""
    shape, lo = (16, 200), (0, 0)
    rng = np.random.default_rng(14)
    rel = np.stack([rng.integers(0, shape[0], size=8), 2 + 28 * np.arange(8)], axis=1).astype(np.int64)
    rel = rel[rng.permutation(8)]
    x = rel.astype(np.float64)
    y = rng.normal(size=(8, 2)) * 30 + 5
    pm, pv = y.mean(0), y.var(0)
    ls, betas = np.array([1.5, 1.5]), rng.uniform(0.5, 2.5, size=2)
    km = np.zeros((2, 8, 8))
    O.update_k(km, x, 0, 8, pv, ls)
    assert max(np.linalg.cond(km[o] + 1e-6 * np.eye(8)) for o in range(2)) < 1e6
    d = dict(x=x, y=y, pm=pm, pv=pv, ls=ls, betas=betas, Kinv=O.invert_k(8, km), rel=rel)
    n_, m_, keep = _pairs_kept(d)
    np.testing.assert_array_equal(keep, n_ == m_)
    pts = G.grid_points(shape, lo)
    ref = O.predict_acquire(x, y, pts, pm, pv, ls, betas, kinv=d["Kinv"])
    for q in (3, 16):
        _check_parity(bo, shape, lo, d, pts, ref, q)

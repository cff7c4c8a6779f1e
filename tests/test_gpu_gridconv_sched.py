"""GPU tests of the pair stage's schedule (bo_gridconv.hip): the list kernel's own offsets
(pstart in closed form from the column buckets), the tau that keep nothing (their T rows are the
list kernel's, they are no items of the accumulate kernel), the class lists that order the
accumulate kernel's items, and the stable column placement at N above one pass of 256 points.

Every case runs in mode="auto-conv" against oracle_np.predict_acquire under the project's tolerance
rule, on a problem with cond(K + 1e-6 I) < 1e6; where and in which order the items are taken may
appear in no value, so repeated calls, graph replays over a garbage workspace and shards are bit
equal."""

import numpy as np
import pytest

from oracle import oracle_np as O
from parity import check_predict, check_topq
import gridconv_model as G
import gridconv_sched_model as S

pytestmark = pytest.mark.gpu

ALL = ("mu", "var", "std_mu", "std_var", "ucb", "acq")
ACC_ROWS = 512          # bo_gridconv.hip: kAccRows
PAIR_DROP = 2.0 ** -100  # kPairDrop


@pytest.fixture(scope="module")
def bo():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import bayesopt_smart_amd as bo
    bo._lib.load()
    return bo


def _cands(bo, shape):
    return bo.predict.CandidateSet.grid([(0, shape[0]), (0, shape[1])])


def _call(bo, d, cands, q, outputs=ALL, mode="auto-conv", offset=0, count=None):
    import torch
    res = bo.predict.predict_acquire(d["x"], d["y"], d["Kinv"], cands, d["pm"], d["pv"], d["ls"], d["betas"],
                                     outputs=outputs, topq=q, offset=offset, count=count, mode=mode)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items() if not k.startswith("_")}


def _excluded(pts, x):
    xs = {tuple(r) for r in np.asarray(x, dtype=np.float64)}
    return np.array([tuple(np.asarray(c, dtype=np.float64)) in xs for c in pts])


def _make(rel, n_obj, seed, ls_range=(1.2, 2.2)):
    """A problem on the integer points `rel` ([n][2]), built like test_gpu_gridconv_pairs.py's: random
    objectives and length scales; with cond(K + 1e-6 I), the largest over the objectives."""
    rng = np.random.default_rng(seed)
    rel = np.asarray(rel, dtype=np.int64)
    n = rel.shape[0]
    assert len({tuple(r) for r in rel}) == n
    x = rel.astype(np.float64)
    y = rng.normal(size=(n, n_obj)) * 30 + 5
    pm, pv = y.mean(0), y.var(0)
    if n == 1:                                       # one point has no spread: any positive prior
        pm, pv = y[0] - 1.0, np.full(n_obj, 4.0)
    ls = rng.uniform(*ls_range, size=n_obj)
    betas = rng.uniform(0.5, 2.5, size=n_obj)
    km = np.zeros((n_obj, n, n))
    O.update_k(km, x, 0, n, pv, ls)
    cond = max(np.linalg.cond(km[o] + 1e-6 * np.eye(n)) for o in range(n_obj))
    return dict(x=x, y=y, pm=pm, pv=pv, ls=ls, betas=betas, Kinv=O.invert_k(n, km), rel=rel, cond=cond)


def _kept_per_tau(d, C):
    """(pairs, kept pairs) per tau = c_n + c_m over the pairs n <= m, by the list kernel's criterion in
    numpy: a pair stays when |w_nm| >= 2^-100 pv for some objective (a non-finite weight stays)."""
    r, c = d["rel"][:, 0], d["rel"][:, 1]
    iu = np.triu_indices(c.size)
    n, m = iu
    d2 = ((r[n] - r[m]) ** 2 + (c[n] - c[m]) ** 2).astype(np.float64)
    keep = np.zeros(n.size, dtype=bool)
    for o in range(len(d["pv"])):
        k = d["Kinv"][o]
        sym = np.where(n == m, k[n, n], k[n, m] + k[m, n])
        w = sym * (d["pv"][o] * d["pv"][o]) * np.exp(0.5 * (-0.5 / d["ls"][o] ** 2) * d2)
        keep |= ~(np.abs(w) < PAIR_DROP * d["pv"][o])
    tau = c[n] + c[m]
    return np.bincount(tau, minlength=2 * C - 1), np.bincount(tau[keep], minlength=2 * C - 1)


def _acc_schedule(shape, n_obj, cus, nrows=None):
    """launch_gridconv's arithmetic: the bound on the accumulate kernel's items, its workgroups of 4
    waves, and whether waves take further items through the tickets (then the class lists are in use)."""
    R, C = shape
    LT = -(-(2 * C - 1) // 16) * 16
    ldr = -(-(R if nrows is None else nrows) // 16) * 16
    items = LT * -(-ldr // ACC_ROWS)
    per_cu = min(4, (160 * 1024) // (32 * R))
    wgs = max(1, min(cus * per_cu // n_obj, -(-items // 4)))
    ngrp = min(wgs, 32)
    return items, wgs, not (items <= 4 * wgs and wgs % ngrp == 0)


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


EDGE_SHAPE = (24, 45)   # 2C - 1 = 89: seven padding tau up to LT = 96


def _edges():
    # two points in column 0 and two in column C - 1 (tau = 0 and 2C - 2, three pairs each), points in
    # neighbouring columns (odd tau), and a few more
    pts = [(2, 0), (9, 0), (5, 44), (17, 44), (11, 20), (13, 21), (20, 7), (3, 30), (21, 31)]
    return EDGE_SHAPE, _make(pts, 2, 21)


def _single():
    return EDGE_SHAPE, _make([(7, 44)], 2, 22)


def _two():
    return EDGE_SHAPE, _make([(7, 0), (8, 1)], 2, 23)


def _two_clusters(shape, n_obj, seed):
    # 40 points in columns 10..25 and 40 in columns 70..85: every cross pair is at least 45 apart
    rng = np.random.default_rng(seed)
    a = rng.choice(30 * 16, size=40, replace=False)
    b = rng.choice(30 * 16, size=40, replace=False)
    pts = np.concatenate([np.stack([5 + a // 16, 10 + a % 16], axis=1), np.stack([20 + b // 16, 70 + b % 16], axis=1)])
    return shape, _make(pts[rng.permutation(80)], n_obj, seed, ls_range=(1.3, 1.7))


def _classes():
    # 380 points scattered over columns 0..259 (a few to a few dozen kept pairs per tau) and 30 in
    # column 290 (one tau with hundreds of kept pairs, a class of its own)
    rng = np.random.default_rng(31)
    lin = rng.choice(64 * 260, size=380, replace=False)
    pts = [(int(v) // 260, int(v) % 260) for v in lin] + [(r, 290) for r in range(2, 62, 2)]
    return (64, 300), _make(pts, 8, 31, ls_range=(1.3, 1.7))


def _narrow(R, n, n_obj, seed):
    rng = np.random.default_rng(seed)
    lin = rng.choice(R * 8, size=n, replace=False)
    return (R, 8), _make(np.stack([lin // 8, lin % 8], axis=1), n_obj, seed, ls_range=(1.2, 1.5))


_BUILDERS = {
    "edges": _edges, "single": _single, "two": _two,
    "clusters-static": lambda: _two_clusters((64, 128), 2, 24),
    "clusters-tickets": lambda: _two_clusters((64, 300), 8, 25),
    "classes": _classes,
    "narrow-257": lambda: _narrow(220, 257, 2, 41),
    "narrow-1025": lambda: _narrow(880, 1025, 1, 42),
}
_PROBLEMS = {}


def _problem(name):
    """(shape, problem, grid points, oracle outputs), computed once per case."""
    if name not in _PROBLEMS:
        shape, d = _BUILDERS[name]()
        pts = G.grid_points(shape, (0, 0))
        ref = O.predict_acquire(d["x"], d["y"], pts, d["pm"], d["pv"], d["ls"], d["betas"], kinv=d["Kinv"])
        _PROBLEMS[name] = (shape, d, pts, ref)
    return _PROBLEMS[name]


def _check_whole(bo, name, q):
    shape, d, pts, ref = _problem(name)
    assert d["cond"] < 1e6
    assert G.conv_planned(shape, d["x"].shape[0], len(d["pm"]), mode="auto-conv")
    cands = _cands(bo, shape)
    out = _call(bo, d, cands, q)
    # the regrouped sum differs from the chunk-major kernel's in the last bits of the variance (were
    # the device flag against the path, the two modes would be equal bit for bit)
    old = _call(bo, d, cands, q, outputs=("var",), mode="auto-noconv")
    assert (out["var"] != old["var"]).any(), "auto-conv ran the chunk-major kernel"
    check_predict(out, ref, d["pv"])
    excl = _excluded(pts, d["x"])
    check_topq(out["top_idx"], ref["acq"], excl, q)
    a = np.where(excl, -np.inf, out["acq"])
    want = np.lexsort((np.arange(a.size), -a))[:q]
    np.testing.assert_array_equal(out["top_idx"], want)
    np.testing.assert_array_equal(out["top_val"], out["acq"][want])
    return shape, d, cands, out


def _assert_bit_equal(runs):
    for r in runs[1:]:
        assert set(r) == set(runs[0])
        for k in runs[0]:
            assert np.array_equal(r[k], runs[0][k]), k


def _garbage_replays(bo, d, cands, q, first):
    """Three replays of one captured graph, the workspace filled with 0x7F before each (counters and
    tickets far past the items, offsets out of range, T entries of 1e306): bit equal to `first`."""
    import torch
    prepared = bo.predict.predict_acquire(d["x"], d["y"], d["Kinv"], cands, d["pm"], d["pv"], d["ls"], d["betas"],
                                          outputs=ALL, topq=q, mode="auto-conv", prepare=True)
    replay = prepared.graphed()
    runs = [first]
    for _ in range(3):
        for t in prepared.res.values():
            if isinstance(t, torch.Tensor):
                t.zero_()
        prepared._ws.fill_(0x7F)
        res = replay()
        torch.cuda.synchronize()
        runs.append({k: res[k].cpu().numpy() for k in first})
    _assert_bit_equal(runs)


def test_offsets_at_the_edges(bo):
    """tau = 0 and tau = 2C - 2 with three pairs each, an odd tau, LT - (2C - 1) = 7 padding tau."""
    shape, d, _, _ = _problem("edges")
    C = shape[1]
    assert (2 * C - 1) % 16 != 0
    cnt = np.diff(S.pstart_closed(d["rel"][:, 1], C, -(-(2 * C - 1) // 16) * 16))
    assert cnt[0] == 3 and cnt[2 * C - 2] == 3 and cnt[41] == 1 and cnt[61] == 1 and (cnt[2 * C - 1:] == 0).all()
    _, _, cands, out = _check_whole(bo, "edges", 5)
    _assert_bit_equal([out, _call(bo, d, cands, 5)])


@pytest.mark.parametrize("name", ["single", "two"])
def test_one_and_two_points(bo, name):
    _check_whole(bo, name, 3)


@pytest.mark.parametrize("name,tickets", [("clusters-static", False), ("clusters-tickets", True)])
def test_tau_that_keeps_nothing_inside_the_band(bo, name, tickets):
    """Two clusters so far apart that every cross pair is dropped: the tau of the cross pairs lie between
    the clusters' own, inside the band of the first column tile, have pairs and keep none.  Their T
    rows are written by the list kernel; left unwritten they would be the 1e306 of the garbage."""
    shape, d, _, _ = _problem(name)
    C = shape[1]
    total, kept = _kept_per_tau(d, C)
    cross = np.arange(80, 111)
    assert total[cross].sum() == 40 * 40 and (kept[cross] == 0).all() and (total[cross] > 0).sum() >= 25
    assert kept[20:51].sum() > 0 and kept[140:171].sum() > 0 and cross.max() < 126      # tile j0 = 0: tau <= 126 + hq
    # the cross pairs are far below the criterion, not at it
    r, c = d["rel"][:, 0].astype(np.float64), d["rel"][:, 1].astype(np.float64)
    far = (c[:, None] < 40) != (c[None, :] < 40)
    d2 = (r[:, None] - r[None, :]) ** 2 + (c[:, None] - c[None, :]) ** 2
    for o in range(len(d["pv"])):
        w = 2 * np.abs(d["Kinv"][o]) * d["pv"][o] * np.exp(-d2 / (4 * d["ls"][o] ** 2))
        assert w[far].max() < 2.0 ** -110
    items, wgs, dyn = _acc_schedule(shape, len(d["pv"]), _cus())
    assert dyn == tickets and (items > 4 * wgs) == tickets
    _, _, cands, first = _check_whole(bo, name, 16)
    _garbage_replays(bo, d, cands, 16, first)


def test_classes(bo):
    """Kept counts over at least six classes on the many-items shape, one class with a single tau and
    one with more than 64 (several rounds of every shard's counter)."""
    shape, d, _, _ = _problem("classes")
    items, wgs, dyn = _acc_schedule(shape, 8, _cus())
    assert items > 4 * wgs and dyn
    _, kept = _kept_per_tau(d, shape[1])
    sizes = np.bincount([S.pair_class(k) for k in kept[kept > 0]])
    assert (sizes > 0).sum() >= 6 and (sizes == 1).any() and sizes.max() > 64, sizes
    _, _, cands, first = _check_whole(bo, "classes", 16)
    _assert_bit_equal([first, _call(bo, d, cands, 16), _call(bo, d, cands, 16)])


def test_shards_cut_a_row(bo):
    """Two shards of the two-cluster case that cut a row: each bit for bit the whole call (a shard has
    its own T and its own items, the same pair list)."""
    shape, d, cands, whole = _check_whole(bo, "clusters-static", 8)
    C = shape[1]
    lo, cut, hi = 2 * C + 5, 30 * C + 17, shape[0] * C - 9
    vals, idxs = [], []
    for a, b in ((lo, cut), (cut, hi)):
        r = _call(bo, d, cands, 8, offset=a, count=b - a)
        for k in ALL:
            np.testing.assert_array_equal(r[k], whole[k][..., a:b], err_msg=f"{k} of shard [{a}, {b})")
        vals.append(r["top_val"])
        idxs.append(r["top_idx"])
    full = _call(bo, d, cands, 8, outputs=("acq",), offset=lo, count=hi - lo)
    v, i = bo.predict.merge_topq(np.concatenate(vals), np.concatenate(idxs), 8)
    np.testing.assert_array_equal(i, full["top_idx"])
    np.testing.assert_array_equal(v, full["top_val"])


def test_band_equals_full_range(bo):
    shape, d, _, _ = _problem("clusters-tickets")
    cands = _cands(bo, shape)
    band = _call(bo, d, cands, 16)
    full = _call(bo, d, cands, 16, mode="auto-conv-full")
    assert set(band) == set(full) == set(ALL) | {"top_idx", "top_val"}
    for k in band:
        np.testing.assert_array_equal(band[k], full[k], err_msg=k)


@pytest.mark.parametrize("name", ["narrow-257", "narrow-1025"])
def test_many_points_per_column(bo, name):
    """8 columns, 32 and 128 points in each on average, N one past 256 and one past 1024: the stable
    placement of the column buckets over more than one pass.  (The oracle does not see the order of a
    bucket; its bits are compared between builds)"""
    shape, d, _, _ = _problem(name)
    assert np.bincount(d["rel"][:, 1], minlength=8).min() >= 16
    _check_whole(bo, name, 8)

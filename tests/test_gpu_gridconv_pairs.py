"""GPU tests of the grid-convolution path's pair stage (bo_gridconv.hip: the schedule of
conv_setup_block, conv_list_kernel, conv_acc_kernel): pair lists that sit in one tau, clustered
points, several row blocks per tau with a ragged last one, the per-objective weights of the shared
list, more items than waves (tickets, the sorted work order with one, two and three passes), and
bit equality across calls, graph replays and shards (the ticket order is in no value).

Every case is compared with oracle_np.predict_acquire under the project's tolerance rule, the way
test_gpu_gridconv.py's test_parity_small_shapes does it, on a problem with cond(K + 1e-6 I) < 1e6."""

import numpy as np
import pytest

from oracle import oracle_np as O
from parity import check_predict, check_topq
import gridconv_model as G

pytestmark = pytest.mark.gpu

ALL = ("mu", "var", "std_mu", "std_var", "ucb", "acq")
ACC_ROWS = 512          # bo_gridconv.hip: kAccRows = 64 kAccRB, the rows of one work item


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


def _make(rel, n_obj, seed):
    """A problem on the integer points `rel` ([n][2]): random objectives, length scales from
    [1.2, 2.2]; returns it with cond(K + 1e-6 I), the largest over the objectives."""
    rng = np.random.default_rng(seed)
    rel = np.asarray(rel, dtype=np.int64)
    n = rel.shape[0]
    assert len({tuple(r) for r in rel}) == n
    x = rel.astype(np.float64)
    y = rng.normal(size=(n, n_obj)) * 30 + 5
    pm, pv = y.mean(0), y.var(0)
    ls = rng.uniform(1.2, 2.2, size=n_obj)
    betas = rng.uniform(0.5, 2.5, size=n_obj)
    km = np.zeros((n_obj, n, n))
    O.update_k(km, x, 0, n, pv, ls)
    cond = max(np.linalg.cond(km[o] + 1e-6 * np.eye(n)) for o in range(n_obj))
    return dict(x=x, y=y, pm=pm, pv=pv, ls=ls, betas=betas, Kinv=O.invert_k(n, km), rel=rel, cond=cond)


def _one_column():
    return (80, 8), _make([(r, 3) for r in range(0, 80, 2)], 2, 11)


def _one_row():
    return (8, 80), _make([(3, c) for c in range(0, 80, 2)], 2, 11)


def _clustered():
    rng = np.random.default_rng(12)
    lin = rng.choice(40 * 40, size=300, replace=False)
    return (64, 256), _make(np.stack([10 + lin // 40, 100 + lin % 40], axis=1), 2, 12)


def _tall():
    shape = (2 * ACC_ROWS + 5, 16)
    rng = np.random.default_rng(13)
    lin = rng.choice(shape[0] * shape[1], size=50, replace=False)
    return shape, _make(np.stack([lin // shape[1], lin % shape[1]], axis=1), 3, 13)


def _eight_objectives():
    shape = (48, 48)
    d = G.lattice_problem(shape, (0, 0), 60, 8, 6)
    km = np.zeros((8, 60, 60))
    O.update_k(km, d["x"], 0, 60, d["pv"], d["ls"])
    d["cond"] = max(np.linalg.cond(km[o] + 1e-6 * np.eye(60)) for o in range(8))
    return shape, d


_BUILDERS = {"one-column": _one_column, "one-row": _one_row, "clustered": _clustered, "tall": _tall,
             "eight-objectives": _eight_objectives}
_PROBLEMS = {}


def _problem(name):
    """(shape, problem, grid points, oracle outputs), computed once per case."""
    if name not in _PROBLEMS:
        shape, d = _BUILDERS[name]()
        pts = G.grid_points(shape, (0, 0))
        ref = O.predict_acquire(d["x"], d["y"], pts, d["pm"], d["pv"], d["ls"], d["betas"], kinv=d["Kinv"])
        _PROBLEMS[name] = (shape, d, pts, ref)
    return _PROBLEMS[name]


def _pairs_per_tau(d, C):
    """Pairs n <= m per tau = c_n + c_m."""
    c = d["rel"][:, 1]
    n = c.size
    iu = np.triu_indices(n)
    return np.bincount(c[iu[0]] + c[iu[1]], minlength=2 * C - 1)


def _assert_new_kernels_ran(bo, d, cands, q, out):
    # the regrouped sum differs from the chunk-major kernel's in the last bits of the variance (were
    # the device flag against the path, the two modes would be equal bit for bit)
    old = _call(bo, d, cands, q, outputs=("var",), mode="auto-noconv")
    assert (out["var"] != old["var"]).any(), "auto-conv ran the chunk-major kernel"


def _check_whole(bo, name, q):
    shape, d, pts, ref = _problem(name)
    assert d["cond"] < 1e6
    assert G.conv_planned(shape, d["x"].shape[0], len(d["pm"]), mode="auto-conv")
    cands = _cands(bo, shape)
    out = _call(bo, d, cands, q)
    _assert_new_kernels_ran(bo, d, cands, q, out)
    check_predict(out, ref, d["pv"])
    excl = _excluded(pts, d["x"])
    check_topq(out["top_idx"], ref["acq"], excl, q)
    # the selection is exactly the order of the call's own acquisition array
    a = np.where(excl, -np.inf, out["acq"])
    want = np.lexsort((np.arange(a.size), -a))[:q]
    np.testing.assert_array_equal(out["top_idx"], want)
    np.testing.assert_array_equal(out["top_val"], out["acq"][want])
    return shape, d, cands, out


def test_one_column(bo):
    """40 points in one column: 820 pairs in a single tau, every other tau empty."""
    shape, d, _, _ = _problem("one-column")
    cnt = _pairs_per_tau(d, shape[1])
    assert cnt[6] == 820 and cnt.sum() == 820
    assert d["cond"] <= 2e2
    _check_whole(bo, "one-column", 3)


def test_one_row(bo):
    """The transpose: every pair of a tau has the same sigma = r_n + r_m."""
    shape, d, _, _ = _problem("one-row")
    assert (d["rel"][:, 0] == 3).all() and _pairs_per_tau(d, shape[1]).sum() == 820
    _check_whole(bo, "one-row", 3)


def test_clustered(bo):
    """300 points of a 40 x 40 block: about 80 non-empty tau, about 1,100 pairs in the longest."""
    shape, d, _, _ = _problem("clustered")
    cnt = _pairs_per_tau(d, shape[1])
    assert (cnt > 0).sum() == 79 and 900 < cnt.max() < 1300
    assert d["cond"] <= 1e5
    _check_whole(bo, "clustered", 16)


def test_eight_objectives(bo):
    """Eight distinct length scales: the per-objective weights of the shared list."""
    shape, d, _, _ = _problem("eight-objectives")
    assert np.unique(d["ls"]).size == 8
    _check_whole(bo, "eight-objectives", 3)


def test_tall_row_blocks_and_shards(bo):
    """2 kAccRows + 5 rows: three row blocks per tau, the last one ragged; then two shards that
    start and end mid-row, the cut inside a row block, bit for bit the whole call."""
    shape, d, cands, whole = _check_whole(bo, "tall", 8)
    C = shape[1]
    lo, cut, hi = 3 * C + 5, 300 * C + 7, shape[0] * C - 9
    assert 0 < cut // C % ACC_ROWS and (hi - 1) // C - cut // C + 1 > ACC_ROWS
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


def _acc_schedule(shape, n_obj, cus, nrows=None):
    """launch_gridconv's arithmetic (bo_gridconv.hip): the accumulate kernel's items, its workgroups of
    4 waves, and whether waves take further items through the tickets (then the work order is sorted)."""
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


def _clustered_tickets():
    rng = np.random.default_rng(14)
    lin = rng.choice(40 * 40, size=300, replace=False)
    return (64, 300), _make(np.stack([10 + lin // 40, 120 + lin % 40], axis=1), 8, 14)


def _long_column():
    # 400 points in one column (80,200 pairs in one tau: three digits of the sort) and 8 elsewhere
    pts = [(r, 150) for r in range(0, 800, 2)] + [(397 + 3 * k, 20 + 35 * k) for k in range(8) if 20 + 35 * k != 150]
    return (800, 300), _make(pts, 8, 15)


_BUILDERS["clustered-tickets"] = _clustered_tickets


def test_tickets_sorted_order_and_graph_replays(bo):
    """8 objectives on (64, 300), 300 points of a 40 x 40 block: more items than waves, so waves take
    further items through the tickets in the sorted work order, and the longest list has two digits
    (two passes of the sort).  Against the oracle; then twice eagerly and three times from one
    captured graph whose workspace is filled with garbage before every replay (a ticket or a T row
    left over from the replay before would show): the schedule and the ticket reset are part of
    the captured sequence, and no value depends on the order the items were taken in."""
    import torch
    shape, d, pts, ref = _problem("clustered-tickets")
    items, wgs, dyn = _acc_schedule(shape, 8, _cus())
    assert items > 4 * wgs and dyn, "no wave takes a second item: the tickets are not exercised"
    assert 256 <= _pairs_per_tau(d, shape[1]).max() < 65536, "not a two-pass sort"
    _, _, cands, first = _check_whole(bo, "clustered-tickets", 16)
    runs = [first, _call(bo, d, cands, 16)]
    prepared = bo.predict.predict_acquire(d["x"], d["y"], d["Kinv"], cands, d["pm"], d["pv"], d["ls"], d["betas"],
                                          outputs=ALL, topq=16, mode="auto-conv", prepare=True)
    replay = prepared.graphed()
    for _ in range(3):
        for t in prepared.res.values():
            if isinstance(t, torch.Tensor):
                t.zero_()
        prepared._ws.fill_(0x7F)             # tickets far past the items, T entries of 1e306
        res = replay()
        torch.cuda.synchronize()
        runs.append({k: res[k].cpu().numpy() for k in runs[0]})
    assert len(runs) == 5
    for r in runs[1:]:
        for k in runs[0]:
            assert np.array_equal(r[k], runs[0][k]), k


def test_long_column_three_pass_sort(bo):
    """400 points in one column of (800, 300), 8 objectives, a shard of 16 rows: 80,200 pairs in one
    tau (three passes of the sort, 157 chunks of the list kernel), 608 items for 512 waves."""
    shape, d = _long_column()
    C = shape[1]
    offset, count = 392 * C + 7, 15 * C + 50
    pts = G.grid_points(shape, (0, 0))[offset:offset + count]       # the oracle on the shard alone
    ref = O.predict_acquire(d["x"], d["y"], pts, d["pm"], d["pv"], d["ls"], d["betas"], kinv=d["Kinv"])
    nrows = (offset + count - 1) // C - offset // C + 1
    items, wgs, dyn = _acc_schedule(shape, 8, _cus(), nrows)
    assert items > 4 * wgs and dyn
    assert _pairs_per_tau(d, C).max() == 80200 >= 65536
    assert d["cond"] < 1e6
    cands = _cands(bo, shape)
    out = _call(bo, d, cands, 8, offset=offset, count=count)
    old = _call(bo, d, cands, 8, outputs=("var",), mode="auto-noconv", offset=offset, count=count)
    assert (out["var"] != old["var"]).any(), "auto-conv ran the chunk-major kernel"
    check_predict(out, ref, d["pv"])
    check_topq(out["top_idx"] - offset, ref["acq"], _excluded(pts, d["x"]), 8)

"""GPU tests of the grid-convolution predict path (bo_gridconv.hip): parity with the oracle under
the project's tolerance rule on small shapes, bit equality across calls / output sets / graph
replay / shards, the device-decided fallback, and the chunk-major kernels' coverage on the shapes
that the default mode now routes to the new path."""

import numpy as np
import pytest

from oracle import oracle_np as O
from parity import check_predict, check_topq
from conftest import predict_fixture
import gridconv_model as G

pytestmark = pytest.mark.gpu

ALL = ("mu", "var", "std_mu", "std_var", "ucb", "acq")


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


def _call(bo, d, cands, q, outputs=ALL, mode="auto-conv", excl=None, offset=0, count=None, x=None):
    import torch
    res = bo.predict.predict_acquire(d["x"] if x is None else x, d["y"], d["Kinv"], cands, d["pm"], d["pv"],
                                     d["ls"], d["betas"], outputs=outputs, topq=q, excl_points=excl,
                                     offset=offset, count=count, mode=mode)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items() if not k.startswith("_")}


def _excluded(pts, x):
    xs = {tuple(r) for r in np.asarray(x, dtype=np.float64)}
    return np.array([tuple(np.asarray(c, dtype=np.float64)) in xs for c in pts])


_PROBLEMS = {}


def _problem(key):
    """(problem, grid points, oracle outputs), computed once per case."""
    if key not in _PROBLEMS:
        shape, lo, n, n_obj, seed = key
        d = G.lattice_problem(shape, lo, n, n_obj, seed)
        pts = G.grid_points(shape, lo)
        ref = O.predict_acquire(d["x"], d["y"], pts, d["pm"], d["pv"], d["ls"], d["betas"], kinv=d["Kinv"])
        _PROBLEMS[key] = (d, pts, ref)
    return _PROBLEMS[key]


LATTICE = ((37, 50), (10 ** 6, -7), 40, 2, 5)


@pytest.mark.parametrize("key,q", [
    (LATTICE, 1), (LATTICE, 3), (LATTICE, 16), (LATTICE, 48),     # neither axis a multiple of 16
    (((48, 48), (0, 0), 60, 8, 6), 3),                            # 8 objectives
    (((40, 64), (-3, 5), 600, 2, 7), 16),                         # dense: pair lists beyond one chunk
    (((9, 20), (0, 0), 1, 2, 8), 3),                              # N = 1
])
def test_parity_small_shapes(bo, key, q):
    shape, lo = key[0], key[1]
    d, pts, ref = _problem(key)
    assert G.conv_planned(shape, key[2], key[3], mode="auto-conv")
    if key[2] == 600:
        c = d["rel"][:, 1]
        cnt = np.bincount(c, minlength=shape[1])
        assert np.convolve(cnt, cnt).max() // 2 > G.PAIR_CHUNK, "no tau with more than one chunk of pairs"
    out = _call(bo, d, _cands(bo, shape, lo), q)
    check_predict(out, ref, d["pv"])
    check_topq(out["top_idx"], ref["acq"], _excluded(pts, d["x"]), q)
    # the selection is exactly the order of the call's own acquisition array
    a = np.where(_excluded(pts, d["x"]), -np.inf, out["acq"])
    want = np.lexsort((np.arange(a.size), -a))[:min(q, int(np.isfinite(a).sum()))]
    np.testing.assert_array_equal(out["top_idx"][:want.size], want)
    np.testing.assert_array_equal(out["top_val"][:want.size], out["acq"][want])
    assert (out["top_idx"][want.size:] == -1).all()


def test_parity_ragged_shard(bo):
    """(64, 256), N = 130, 3 objectives, a shard that starts and ends mid-row."""
    key = ((64, 256), (0, 0), 130, 3, 9)
    shape, lo = key[0], key[1]
    d, pts, ref = _problem(key)
    offset, count = 3 * 256 + 5, 41 * 256 + 77
    out = _call(bo, d, _cands(bo, shape, lo), 8, offset=offset, count=count)
    sl = slice(offset, offset + count)
    check_predict(out, {k: (ref[k][sl] if k == "acq" else ref[k][:, sl]) for k in ALL}, d["pv"])
    check_topq(out["top_idx"] - offset, ref["acq"][sl], _excluded(pts[sl], d["x"]), 8)


@pytest.mark.parametrize("q", [1, 3, 16, 48])
def test_topq_exclusion_at_the_top(bo, q):
    """beta = 0 and short length scales: the acquisition peaks AT the best training points, so the
    evaluated points lead the order and the selection must step over them."""
    rng = np.random.default_rng(25)      # (a seed whose best candidate is an evaluated point)
    side, n = 96, 40
    lin = rng.choice(side * side, size=n, replace=False)
    x = np.stack([lin // side, lin % side], axis=1).astype(np.float64)
    y = np.zeros((n, 2))
    y[:6, 0] = [1000, 900, 800, 700, 600, 500]
    y[:6, 1] = [50, 40, 30, 20, 10, 5]
    y[6:] = rng.normal(size=(n - 6, 2))
    pm, pv = y.mean(0), y.var(0)
    ls, betas = np.array([3.0, 3.0]), np.zeros(2)
    km = np.zeros((2, n, n))
    O.update_k(km, x, 0, n, pv, ls)
    d = dict(x=x, y=y, pm=pm, pv=pv, ls=ls, betas=betas, Kinv=O.invert_k(n, km))
    out = _call(bo, d, _cands(bo, (side, side), (0, 0)), q, outputs=("acq",))
    acq = out["acq"]
    excl = np.zeros(side * side, dtype=bool)
    excl[lin] = True
    assert excl[np.lexsort((np.arange(side * side), -acq))[:q]].any(), "no evaluated point at the top"
    want = np.lexsort((np.arange(side * side), -np.where(excl, -np.inf, acq)))[:q]
    np.testing.assert_array_equal(out["top_idx"], want)
    np.testing.assert_array_equal(out["top_val"], acq[want])


def test_excl_points_differ_from_x_train(bo):
    d, pts, ref = _problem(LATTICE)
    shape, lo = LATTICE[0], LATTICE[1]
    order = np.argsort(-ref["acq"], kind="stable")
    # exclude the reference's three best candidates and nothing else (not the training points)
    excl_pts = pts[order[:3]].astype(np.float64)
    out = _call(bo, d, _cands(bo, shape, lo), 5, outputs=("acq",), excl=excl_pts)
    mask = np.zeros(pts.shape[0], dtype=bool)
    mask[order[:3]] = True
    want = np.lexsort((np.arange(mask.size), -np.where(mask, -np.inf, out["acq"])))[:5]
    np.testing.assert_array_equal(out["top_idx"], want)
    check_topq(out["top_idx"], ref["acq"], mask, 5)


def test_bit_equality_calls_outputs_graph(bo):
    import torch
    d, pts, ref = _problem(LATTICE)
    cands = _cands(bo, LATTICE[0], LATTICE[1])
    a = _call(bo, d, cands, 3)
    b = _call(bo, d, cands, 3)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    # the new kernels did run: the regrouped sum differs from the chunk-major kernel's in the last
    # bits of the variance (were the device flag against the path, the two modes would be equal
    # bit for bit, as in test_fallback_decided_on_the_device)
    old = _call(bo, d, cands, 3, mode="auto-noconv")
    assert (a["var"] != old["var"]).any(), "auto-conv ran the chunk-major kernel"
    only = _call(bo, d, cands, 3, outputs=("acq",))
    np.testing.assert_array_equal(only["acq"], a["acq"])
    np.testing.assert_array_equal(only["top_idx"], a["top_idx"])
    np.testing.assert_array_equal(only["top_val"], a["top_val"])
    prepared = bo.predict.predict_acquire(d["x"], d["y"], d["Kinv"], cands, d["pm"], d["pv"], d["ls"], d["betas"],
                                          outputs=ALL, topq=3, mode="auto-conv", prepare=True)
    replay = prepared.graphed()
    for t in prepared.res.values():
        if isinstance(t, torch.Tensor):
            t.zero_()
    res = replay()
    torch.cuda.synchronize()
    for k in a:
        np.testing.assert_array_equal(res[k].cpu().numpy(), a[k])


def test_bit_equality_shards(bo):
    key = ((64, 256), (0, 0), 130, 3, 9)
    d, pts, ref = _problem(key)
    cands = _cands(bo, key[0], key[1])
    total = key[0][0] * key[0][1]
    full = _call(bo, d, cands, 16, outputs=("acq",))
    bounds = [0, 1000, 1000 + 256 * 7 + 3, 9001, total]
    vals, idxs, accs = [], [], []
    for lo_, hi_ in zip(bounds[:-1], bounds[1:]):
        r = _call(bo, d, cands, 16, outputs=("acq",), offset=lo_, count=hi_ - lo_)
        vals.append(r["top_val"])
        idxs.append(r["top_idx"])
        accs.append(r["acq"])
    np.testing.assert_array_equal(np.concatenate(accs), full["acq"])
    v, i = bo.predict.merge_topq(np.concatenate(vals), np.concatenate(idxs), 16)
    np.testing.assert_array_equal(i, full["top_idx"])
    np.testing.assert_array_equal(v, full["top_val"])


@pytest.mark.parametrize("case", ["half", "outside"])
def test_fallback_decided_on_the_device(bo, case):
    """A training point off the grid (one coordinate at x + 0.5) or outside the grid box: the call
    planned for the new path runs the chunk-major kernel, bit for bit the auto-noconv result."""
    shape, lo = LATTICE[0], LATTICE[1]
    base = _problem(LATTICE)[0]
    x = base["x"].copy()
    if case == "half":
        x[7, 1] += 0.5
    else:
        x[7, 0] = lo[0] + shape[0] + 2
    n = x.shape[0]
    km = np.zeros((2, n, n))
    O.update_k(km, x, 0, n, base["pv"], base["ls"])
    assert max(np.linalg.cond(km[o] + 1e-6 * np.eye(n)) for o in range(2)) < 1e6
    d = dict(base, x=x, Kinv=O.invert_k(n, km))
    pts = G.grid_points(shape, lo)
    ref = O.predict_acquire(x, d["y"], pts, d["pm"], d["pv"], d["ls"], d["betas"], kinv=d["Kinv"])
    cands = _cands(bo, shape, lo)
    conv = _call(bo, d, cands, 16)
    noconv = _call(bo, d, cands, 16, mode="auto-noconv")
    for k in conv:
        np.testing.assert_array_equal(conv[k], noconv[k])
    check_predict(conv, ref, d["pv"])
    check_topq(conv["top_idx"], ref["acq"], _excluded(pts, x), 16)


# ---- the chunk-major (SEP + UPPER) kernels on the shapes that "auto" now sends to the new path


@pytest.mark.parametrize("q", [3, 16])
def test_noconv_implicit_grid_golden(bo, q):
    d = predict_fixture("g1_grid")
    shape = (int(d["grid_shape"][0]), int(d["grid_shape"][1]))
    cands = bo.predict.CandidateSet.grid([(0, shape[0]), (0, shape[1])])
    out = _call(bo, d, cands, q, mode="auto-noconv")
    check_predict(out, d, d["pv"])
    check_topq(out["top_idx"], d["acq"], _excluded(d["cand"], d["x"]), q)
    np.testing.assert_array_equal(cands.points(out["top_idx"][:3]), d["select_q3"])


@pytest.mark.parametrize("shape,n,n_obj,offset", [((16, 1024), 480, 4, 0), ((16, 1024), 300, 3, 3 * 1024 + 48)])
def test_noconv_row_factor_paths(bo, shape, n, n_obj, offset):
    rng = np.random.default_rng(n)
    total = shape[0] * shape[1]
    lin = rng.choice(total, size=n, replace=False)
    x = np.stack(np.unravel_index(lin, shape), axis=1).astype(np.float64)
    y = rng.normal(size=(n, n_obj)) * 30 + 5
    pm, pv = y.mean(0), y.var(0)
    ls, betas = rng.uniform(1.5, 2.5, size=n_obj), rng.uniform(0.5, 2.5, size=n_obj)
    km = np.zeros((n_obj, n, n))
    O.update_k(km, x, 0, n, pv, ls)
    d = dict(x=x, y=y, pm=pm, pv=pv, ls=ls, betas=betas, Kinv=O.invert_k(n, km))
    cands = bo.predict.CandidateSet.grid([(0, s) for s in shape])
    count = min(total - offset, 8192)
    out = _call(bo, d, cands, 8, outputs=("mu", "var", "acq"), mode="auto-noconv", offset=offset, count=count)
    sub = np.unique(np.r_[np.arange(0, 300), rng.choice(count, 700, replace=False)])
    pts = np.stack(np.unravel_index(offset + sub, shape), axis=1).astype(np.int64)
    ref = O.predict_acquire(x, y, pts, pm, pv, ls, betas, kinv=d["Kinv"])
    check_predict({"mu": out["mu"][:, sub], "var": out["var"][:, sub], "acq": out["acq"][sub]},
                  {k: ref[k] for k in ("mu", "var", "acq")}, pv)
    shard_pts = np.stack(np.unravel_index(offset + np.arange(count), shape), axis=1)
    check_topq(out["top_idx"] - offset, out["acq"], _excluded(shard_pts, x), 8)
    # and the new path on the same call agrees within the rule's bound on both sides
    conv = _call(bo, d, cands, 8, outputs=("mu", "var", "acq"), mode="auto-conv", offset=offset, count=count)
    check_predict({"mu": conv["mu"][:, sub], "var": conv["var"][:, sub], "acq": conv["acq"][sub]},
                  {k: ref[k] for k in ("mu", "var", "acq")}, pv)


@pytest.mark.parametrize("q", [1, 2, 3, 4, 5])
def test_noconv_lane_topq_exclusion_at_the_top(bo, q):
    """test_grid_topq_exclusion_at_the_top's shape on the chunk-major kernel: the lanes' own lists
    (q <= 4) and the wave-shared list (q = 5)."""
    rng = np.random.default_rng(21 + q)
    side, n = 256, 40
    lin = rng.choice(side * side, size=n, replace=False)
    x = np.stack([lin // side, lin % side], axis=1).astype(np.float64)
    y = np.zeros((n, 2))
    y[:6, 0] = [1000, 900, 800, 700, 600, 500]
    y[:6, 1] = [50, 40, 30, 20, 10, 5]
    y[6:] = rng.normal(size=(n - 6, 2))
    pm, pv = y.mean(0), y.var(0)
    ls, betas = np.array([3.0, 3.0]), np.zeros(2)
    km = np.zeros((2, n, n))
    O.update_k(km, x, 0, n, pv, ls)
    d = dict(x=x, y=y, pm=pm, pv=pv, ls=ls, betas=betas, Kinv=O.invert_k(n, km))
    out = _call(bo, d, _cands(bo, (side, side), (0, 0)), q, outputs=("acq",), mode="auto-noconv")
    excl = np.zeros(side * side, dtype=bool)
    excl[lin] = True
    order_all = np.lexsort((np.arange(side * side), -out["acq"]))
    assert excl[order_all[:q]].any(), "no evaluated point at the top: the case is not exercised"
    want = np.lexsort((np.arange(side * side), -np.where(excl, -np.inf, out["acq"])))[:q]
    np.testing.assert_array_equal(out["top_idx"], want)
    np.testing.assert_array_equal(out["top_val"], out["acq"][want])


@pytest.mark.parametrize("n", [518, 530, 541])
def test_noconv_grid_part_lane_topq_vs_cpu(bo, n):
    """test_grid_part_lane_topq_vs_cpu on the chunk-major kernel: N off a multiple of 32 (the PART
    instantiation, 1 / 3 / 3 live k-step pairs in the peeled chunk) with q = 3 (the lane lists),
    every candidate of the 512 x 1024 grid against the CPU reference (oracle/cpu_ref.c; the same
    cached arrays as that test's) and the top-3 judged on the CPU acquisition array."""
    from fullref import cpu_full, grid_points_2d
    rng = np.random.default_rng(n)
    rows, side = 512, 1024
    lin = rng.choice(rows * side, size=n, replace=False)
    x = np.stack([lin // side, lin % side], axis=1).astype(np.float64)
    y = np.stack([-((x[:, 0] - 150) ** 2) + 100, -((x[:, 1] - 150) ** 2) + 20], axis=1)
    pm, pv = y.mean(0), y.var(0)
    ls, betas = np.array([20.0, 20.0]), np.array([2.0, 2.0])
    km = np.zeros((2, n, n))
    O.update_k(km, x, 0, n, pv, ls)
    d = dict(x=x, y=y, pm=pm, pv=pv, ls=ls, betas=betas, Kinv=O.invert_k(n, km))
    cands = bo.predict.CandidateSet.grid([(0, rows), (0, side)])
    got = _call(bo, d, cands, 3, outputs=("mu", "var", "acq"), mode="auto-noconv")
    ref = cpu_full(("grid_part", n), x, y, grid_points_2d(rows, side), d["Kinv"], pm, pv, ls, betas)
    check_predict({k: got[k] for k in ("mu", "var", "acq")}, ref, pv)
    excl = np.zeros(rows * side, dtype=bool)
    excl[lin] = True
    check_topq(got["top_idx"], ref["acq"], excl, 3)


def test_noconv_c2_grid_ucb(bo):
    """test_gpu_configs.py's test_c2_grid_ucb[auto] on the chunk-major kernel (N = 128: the small-N
    kernel, the lane lists): every candidate of C2 against the CPU reference (the same cached
    arrays), the per-objective UCB array included."""
    import test_gpu_configs as C
    from fullref import cpu_full, grid_points_2d
    rng = np.random.default_rng(0)
    side = 512
    lin = rng.choice(side * side, size=128, replace=False)
    x = np.stack([lin // side, lin % side], axis=1).astype(np.float64)
    d = C.problem(x, C.toy_function(x), 20.0, 2.0)
    cands = bo.predict.CandidateSet.grid([(0, side), (0, side)])
    out = _call(bo, d, cands, 3, outputs=("mu", "var", "ucb", "acq"), mode="auto-noconv")
    ref = cpu_full("C2", x, d["y"], grid_points_2d(side, side), d["Kinv"], d["pm"], d["pv"], d["ls"],
                   d["betas"])
    check_predict({k: out[k] for k in ("mu", "var", "ucb", "acq")}, ref, d["pv"])
    excl = np.zeros(side * side, dtype=bool)
    excl[lin] = True
    check_topq(out["top_idx"], ref["acq"], excl, 3)


def test_noconv_full_size_c3(bo):
    """test_full_size_c3_properties' default-mode part on the chunk-major kernel: every candidate of
    C3 against the CPU reference (the same cached arrays), q = 16, deterministic across output
    sets."""
    from fullref import cpu_full, grid_points_2d
    rng = np.random.default_rng(0)
    side = 1024
    lin = rng.choice(side * side, size=512, replace=False)
    x = np.stack([lin // side, lin % side], axis=1).astype(np.float64)
    y = np.stack([-(x[:, 0] - 150) ** 2 + 100, -(x[:, 1] - 150) ** 2 + 20], axis=1)
    pm, pv = y.mean(0), y.var(0)
    ls, betas = np.array([20.0, 20.0]), np.array([2.0, 2.0])
    km = np.zeros((2, 512, 512))
    O.update_k(km, x, 0, 512, pv, ls)
    d = dict(x=x, y=y, Kinv=O.invert_k(512, km), pm=pm, pv=pv, ls=ls, betas=betas)
    cands = bo.predict.CandidateSet.grid([(0, side), (0, side)])
    out = _call(bo, d, cands, 16, outputs=("mu", "var", "acq"), mode="auto-noconv")
    out2 = _call(bo, d, cands, 16, outputs=("acq",), mode="auto-noconv")
    np.testing.assert_array_equal(out["acq"], out2["acq"])
    np.testing.assert_array_equal(out["top_idx"], out2["top_idx"])
    excl = np.zeros(side * side, dtype=bool)
    excl[lin] = True
    ref = cpu_full("C3", x, y, grid_points_2d(side, side), d["Kinv"], pm, pv, ls, betas)
    check_predict({k: out[k] for k in ("mu", "var", "acq")}, ref, pv)
    check_topq(out["top_idx"], ref["acq"], excl, 16)


def _sweep_cases_on_the_new_path():
    """The 2-D grid cases of test_gpu_sweep.py that the plan's gate sends to the new path."""
    import test_gpu_sweep as S
    out = []
    for case in S.CASES:
        cid, kind, geo, n, n_obj, q, mode, offset, count = case
        if kind != "grid" or len(geo) != 2 or mode != "auto":
            continue
        total = geo[0] * geo[1]
        cnt = min(S._count(n, n_obj, total - offset) if count is None else count, total - offset)
        if G.conv_planned(tuple(geo), n, n_obj, offset, cnt):
            out.append(case)
    return out


@pytest.mark.parametrize("case", _sweep_cases_on_the_new_path(), ids=lambda c: c[0])
def test_noconv_sweep_cases(bo, case):
    """test_gpu_sweep.py's test_kernel_variant_vs_cpu on the chunk-major kernel, for the cases whose
    default mode now takes the new path: the same problem, the CPU reference on every candidate of
    the shard, the top-q judged on the reference acquisition."""
    import test_gpu_sweep as S
    from oracle import cpu_ref
    cid, kind, geo = case[:3]
    cs = S._cand_set(bo, kind, geo, sum(map(ord, cid)))
    p = S.make_case(case, lambda idx: np.asarray(cs.points(idx), dtype=np.float64))
    off, cnt, q = p["offset"], p["count"], p["q"]
    d = dict(x=p["x"], y=p["y"], Kinv=p["kinv"], pm=p["pm"], pv=p["pv"], ls=p["ls"], betas=p["betas"])
    got = _call(bo, d, cs, q, outputs=("mu", "var", "acq"), mode="auto-noconv", offset=off, count=cnt)
    pts = np.asarray(cs.points(np.arange(off, off + cnt)), dtype=np.float64)
    ref = cpu_ref.predict_acquire(p["x"], p["y"], pts, p["kinv"], p["pm"], p["pv"], p["ls"], p["betas"])
    excl = _excluded(pts, p["x"])
    check_predict({k: got[k] for k in ("mu", "var", "acq")}, ref, p["pv"])
    check_topq(got["top_idx"] - off, ref["acq"], excl, q)

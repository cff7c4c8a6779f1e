"""The f64 predict paths against the extended-precision reference of tests/exact_ref.py, under its
rounding-error bound  |d var| <= Cq u S_q + 2u pv,  |d mu| <= Cmu u S_mu + 2u |mu|  (u = 2^-53; the
scales, the derived constants and what the bound leaves out -- the 2^-100 pv pair drop and the 2^-128
table flush, both many orders below 2u pv -- are stated in that module's docstring).  K^-1 is data: the
array handed to the device is the reference's A, so the bound holds at any cond(K), and the cases go
from cond 12 to 5e15 (the fitted loop's regime) and onto the device's own non-symmetric LU inverse.

Paths: the grid-convolution path at every contraction tile width (BO_CONV_TILE = 1, 2, 4) and without
its band, the chunk-major kernels (small, SEP, UPPER, dense, direct on Sobol / f64 / i64 sets, GROWS)
and the unfused bo_update_k_star -> bo_update_mean_variance.  Each case computes its reference once.
Every test prints the worst err / (u scale) per output (pytest -s)."""

import numpy as np
import pytest

import exact_ref as X
import gridconv_model as G
from oracle import oracle_np as O
from parity import check_topq
from test_gpu_gridconv_tiles import _tile, _two_sided

pytestmark = pytest.mark.gpu

Q = 16
BUDGET = 3e8               # candidates x N^2 x n_obj scored by the reference per case
CONV_MODES = [("auto-conv", "1"), ("auto-conv", "2"), ("auto-conv", "4")]
ALL_MODES = CONV_MODES + [("auto-conv-full", None), ("auto-noconv", None), ("dense", None), ("auto-exp", None)]


@pytest.fixture(scope="module")
def bo():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import bayesopt_smart_amd as bo
    bo._lib.load()
    return bo


def _path(mode):
    return "gridconv" if mode.startswith("auto-conv") else "chunk-major"


def _call(bo, d, cands, mode, tile=None, q=Q, outputs=X.OUTPUTS, offset=0, count=None):
    import torch
    with _tile(tile):
        res = bo.predict.predict_acquire(d["x"], d["y"], d["Kinv"], cands, d["pm"], d["pv"], d["ls"], d["betas"],
                                         outputs=outputs, topq=q, offset=offset, count=count, mode=mode)
        torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items() if not k.startswith("_")}


def _excluded(pts, x):
    xs = {tuple(r) for r in np.asarray(x, dtype=np.float64)}
    return np.array([tuple(np.asarray(c, dtype=np.float64)) in xs for c in pts])


# ---- grid cases

def _case_d():
    """64 x 96, N = 300 random grid points, ls = 20, the objectives of test_noconv_full_size_c3: the
    fitted loop's regime (cond(K + 1e-6 I) 5e15)."""
    rng = np.random.default_rng(0)
    R, C, n = 64, 96, 300
    lin = rng.choice(R * C, size=n, replace=False)
    x = np.stack([lin // C, lin % C], axis=1).astype(np.float64)
    y = np.stack([-(x[:, 0] - 150) ** 2 + 100, -(x[:, 1] - 150) ** 2 + 20], axis=1)
    d = dict(x=x, y=y, pm=y.mean(0), pv=y.var(0), betas=np.array([2.0, 2.0]))
    return X.relength(d, (20.0, 20.0))


def _sample_d(d, shape):
    """Every training point and its 8 neighbours, the corners of every 16 x 16 wave tile (the first and
    last candidate of each tile row and column), the grid's first and last 64 candidates, 256 random."""
    R, C = shape
    r, c = d["x"][:, 0].astype(np.int64), d["x"][:, 1].astype(np.int64)
    idx = [((r + dr).clip(0, R - 1)) * C + (c + dc).clip(0, C - 1) for dr in (-1, 0, 1) for dc in (-1, 0, 1)]
    edge_r = np.unique(np.r_[np.arange(0, R, 16), np.arange(15, R, 16), R - 1])
    edge_c = np.unique(np.r_[np.arange(0, C, 16), np.arange(15, C, 16), C - 1])
    idx.append((edge_r[:, None] * C + edge_c[None, :]).ravel())
    idx.append(np.r_[np.arange(64), np.arange(R * C - 64, R * C)])
    idx.append(np.random.default_rng(1).choice(R * C, 256, replace=False))
    return np.unique(np.concatenate(idx))


GRID_CASES = {
    # name: (problem, shape, lo, sample (None: every candidate))
    "G-a": lambda: X.lattice_case("a") + (None,),
    "G-b": lambda: X.lattice_case("b") + (None,),
    "G-c": lambda: X.lattice_case("c") + (None,),
    "G-d": lambda: (lambda d: (d, (64, 96), (0, 0), _sample_d(d, (64, 96))))(_case_d()),
    "G-e": lambda: (dict(_two_sided(3, [1.8, 2.5, 3.4], 12), cond=float("nan")), (40, 200), (0, 0), None),
    "G-f": lambda: (dict(G.lattice_problem((48, 48), (0, 0), 60, 8, 6), cond=float("nan")), (48, 48), (0, 0), None),
    "G-g": lambda: (dict(G.lattice_problem((9, 20), (0, 0), 1, 2, 8), cond=float("nan")), (9, 20), (0, 0), None),
}
_GRID = {}


def _grid(name):
    """(problem, shape, lo, scored indices, their points, reference), the reference computed once."""
    if name not in _GRID:
        d, shape, lo, sample = GRID_CASES[name]()
        total = shape[0] * shape[1]
        idx = (np.arange(total) if sample is None else sample)[::X.SUBSAMPLE]
        pts = G.grid_points(shape, lo)[idx]
        # (G-d's prescribed sample is 2454 candidates at N = 300: 4.4e8, 2.2 s of reference, once)
        assert idx.size * d["x"].shape[0] ** 2 * len(d["pm"]) <= (1.5 if name == "G-d" else 1.0) * BUDGET
        ref = X.exact_predict(d["x"], d["y"], d["Kinv"], d["pm"], d["pv"], d["ls"], d["betas"], pts)
        _GRID[name] = (d, shape, lo, idx, pts, ref)
    return _GRID[name]


def _take(arrs, idx):
    return {k: np.asarray(v)[..., idx] for k, v in arrs.items()}


GRID_RUNS = [(c, m, t) for c in ("G-a", "G-b") for m, t in ALL_MODES] + \
            [(c, m, t) for c in ("G-c", "G-d") for m, t in CONV_MODES + [("auto-noconv", None)]] + \
            [(c, m, t) for c in ("G-e", "G-f", "G-g") for m, t in CONV_MODES]


@pytest.mark.parametrize("case,mode,tile", GRID_RUNS, ids=[f"{c}-{m}" + (f"-tile{t}" if t else "") for c, m, t in GRID_RUNS])
def test_grid_paths(bo, case, mode, tile):
    d, shape, lo, idx, pts, ref = _grid(case)
    n, n_obj = d["x"].shape[0], len(d["pm"])
    if mode.startswith("auto-conv"):
        assert G.conv_planned(shape, n, n_obj, mode="auto-conv")
    cands = bo.predict.CandidateSet.grid([(lo[0], lo[0] + shape[0]), (lo[1], lo[1] + shape[1])])
    out = _call(bo, d, cands, mode, tile)
    cq, cmu = X.path_constants(_path(mode), n, shape[1], 2)
    got = _take({k: out[k] for k in X.OUTPUTS}, idx)
    _, tol = X.check_exact(got, ref, d["pv"], d["betas"], cq, cmu,
                           f"{case} {mode} tile {tile} (N {n}, cond {d['cond']:.1e})")
    if idx.size == shape[0] * shape[1]:
        check_topq(out["top_idx"], ref["acq"], _excluded(pts, d["x"]), Q, tol=tol["acq"])


@pytest.mark.parametrize("mode", ["auto-conv", "auto-noconv"])
def test_grid_ragged_shard(bo, mode):
    """G-c from the middle of row 3 to the middle of row 33."""
    d, shape, lo, idx, pts, ref = _grid("G-c")
    offset, count = 3 * 64 + 5, 30 * 64 + 13
    keep = (idx >= offset) & (idx < offset + count)
    cands = bo.predict.CandidateSet.grid([(lo[0], lo[0] + shape[0]), (lo[1], lo[1] + shape[1])])
    out = _call(bo, d, cands, mode, offset=offset, count=count)
    cq, cmu = X.path_constants(_path(mode), d["x"].shape[0], shape[1], 2)
    sub = _take({k: v for k, v in ref.items() if k not in ("m_ext", "q_ext")}, keep)
    got = _take({k: out[k] for k in X.OUTPUTS}, idx[keep] - offset)
    _, tol = X.check_exact(got, sub, d["pv"], d["betas"], cq, cmu, f"G-c shard {mode}")
    if keep.sum() == count:
        check_topq(out["top_idx"] - offset, sub["acq"], _excluded(pts[keep], d["x"]), Q, tol=tol["acq"])


@pytest.mark.parametrize("mode", ["auto-conv", "auto-noconv"])
def test_device_inverse(bo, mode):
    """The loop's own situation above cond 1e6: device update_k -> invert_k on the blocked LU (lu_hint)
    on G-c's points at ls = 14; the device's non-symmetric K^-1, copied back, is the reference's A."""
    import torch
    key = "dev-kinv"
    base, shape, lo = X.lattice_case("c")
    n, n_obj = base["x"].shape[0], len(base["pm"])
    if key not in _GRID:
        km = torch.zeros((n_obj, n, n), dtype=torch.float64, device="cuda")
        bo.kernels.update_k(km, torch.tensor(base["x"], device="cuda"), 0, n, base["pv"], base["ls"])
        taken = []
        kinv = bo.kernels.invert_k(n, km, lu_hint=[True] * n_obj, paths=taken).cpu().numpy()
        assert taken == [1] * n_obj, taken
        assert np.isfinite(kinv).all()
        d = dict(base, Kinv=kinv)
        idx = np.arange(shape[0] * shape[1])[::X.SUBSAMPLE]
        pts = G.grid_points(shape, lo)[idx]
        ref = X.exact_predict(d["x"], d["y"], kinv, d["pm"], d["pv"], d["ls"], d["betas"], pts)
        _GRID[key] = (d, idx, pts, ref)
    d, idx, pts, ref = _GRID[key]
    asym = max(float(np.abs(a - a.T).max() / np.abs(a).max()) for a in d["Kinv"])
    cands = bo.predict.CandidateSet.grid([(lo[0], lo[0] + shape[0]), (lo[1], lo[1] + shape[1])])
    out = _call(bo, d, cands, mode)
    cq, cmu = X.path_constants(_path(mode), n, shape[1], 2)
    _, tol = X.check_exact(_take({k: out[k] for k in X.OUTPUTS}, idx), ref, d["pv"], d["betas"], cq, cmu,
                           f"device K^-1 (LU, asymmetry {asym:.1e}) {mode}")
    if idx.size == shape[0] * shape[1]:
        check_topq(out["top_idx"], ref["acq"], _excluded(pts, d["x"]), Q, tol=tol["acq"])


def test_unfused_abi(bo):
    """bo_update_k_star -> bo_update_mean_variance on G-b (the materialised K*, the dense chain)."""
    import torch
    d, shape, lo, idx, pts, ref = _grid("G-b")
    n, n_obj = d["x"].shape[0], len(d["pm"])
    space = torch.tensor(G.grid_points(shape, lo), device="cuda")
    m = space.shape[0]
    ks = torch.zeros((n_obj, n, m), dtype=torch.float64, device="cuda")
    xd, yd = torch.tensor(d["x"], device="cuda"), torch.tensor(d["y"], device="cuda")
    kinv = torch.tensor(d["Kinv"], device="cuda")
    bo.kernels.update_k_star(ks, xd, space, 0, n, d["pv"], d["ls"])
    mu = torch.empty((n_obj, m), dtype=torch.float64, device="cuda")
    var = torch.empty((n_obj, m), dtype=torch.float64, device="cuda")
    bo.kernels.update_mean(mu, ks, kinv, yd, d["pm"], n)
    bo.kernels.update_variance(var, ks, kinv, d["pv"], n)
    torch.cuda.synchronize()
    cq, cmu = X.path_constants("chunk-major", n, shape[1], 2)
    X.check_exact(_take({"mu": mu.cpu().numpy(), "var": var.cpu().numpy()}, idx), ref, d["pv"], d["betas"],
                  cq, cmu, "G-b unfused")


# ---- the chunk-major kernels off the 2-D grid: cases of tests/test_gpu_sweep.py

SWEEP_IDS = ["sobol4-n260-q7", "sobol5-n65-small-q2", "f64-d2-n90-q3", "i64-d7-n410-q4", "grid3d-n150-q3",
             "grid-n545-q1", "sobol6-nobj6-n300-q5", "grid8d-grows-n1700-q3"]


def _cond(x, pv, ls):
    """cond(K / pv + 1e-6 I) of objective 0 (printed, not asserted)."""
    km = np.zeros((1, x.shape[0], x.shape[0]))
    O.update_k(km, x, 0, x.shape[0], pv[:1], ls[:1])
    ev = np.abs(np.linalg.eigvalsh(km[0] / pv[0] + 1e-6 * np.eye(x.shape[0])))
    return float(ev.max() / ev.min())


@pytest.mark.parametrize("scale", [1, 4], ids=["ls1", "ls4"])
@pytest.mark.parametrize("cid", SWEEP_IDS)
def test_sweep_cases(bo, cid, scale):
    """The sweep's problem at its own length scale and at 4x (K^-1 rebuilt by O.invert_k), the count cut
    to the reference's budget."""
    import test_gpu_sweep as S
    case = next(c for c in S.CASES if c[0] == cid)
    kind, geo = case[1], case[2]
    cs = S._cand_set(bo, kind, geo, sum(map(ord, cid)))
    p = S.make_case(case, lambda i: np.asarray(cs.points(i), dtype=np.float64))
    n, n_obj = p["x"].shape[0], len(p["pm"])
    d = dict(x=p["x"], y=p["y"], pm=p["pm"], pv=p["pv"], ls=p["ls"], betas=p["betas"], Kinv=p["kinv"])
    if scale != 1:
        ls = scale * p["ls"]
        km = np.zeros((n_obj, n, n))
        O.update_k(km, d["x"], 0, n, d["pv"], ls)
        d = dict(d, ls=ls, Kinv=O.invert_k(n, km))
    off = p["offset"]
    cap = 48 if cid.startswith("grid8d") else int(BUDGET / (n * n * n_obj))
    count = min(p["count"], cap)
    mode = "auto-noconv" if cid == "grid-n545-q1" else p["mode"]
    out = _call(bo, d, cs, mode, q=p["q"], offset=off, count=count)
    idx = np.arange(off, off + count)[::X.SUBSAMPLE]
    pts = cs.points(idx)                      # exactly the device's values (int64 on a grid)
    ref = X.exact_predict(d["x"], d["y"], d["Kinv"], d["pm"], d["pv"], d["ls"], d["betas"], pts)
    dim = d["x"].shape[1]
    cq, cmu = X.path_constants("chunk-major", n, geo[-1] if kind == "grid" else 0, dim)
    label = f"{cid} x{scale} {sorted(S.plan_path(case[:8] + (count,)))} count {count} cond0 {_cond(d['x'], d['pv'], d['ls']):.1e}"
    _, tol = X.check_exact(_take({k: out[k] for k in X.OUTPUTS}, idx - off), ref, d["pv"], d["betas"], cq, cmu, label)
    # the numpy oracle on the same case, for the comparison of DESIGN §5 (printed, not asserted)
    o = O.predict_acquire(d["x"], d["y"], pts, d["pm"], d["pv"], d["ls"], d["betas"], kinv=d["Kinv"])
    ro = X.ratios({k: o[k] for k in ("mu", "var")}, ref, X.tolerances(ref, d["pv"], d["betas"], 1.0, 1.0))
    print(f"    oracle_np on {cid} x{scale}: mu {ro['mu']:.3g}, var {ro['var']:.3g}")
    if idx.size == count:
        check_topq(out["top_idx"] - off, ref["acq"], _excluded(pts, d["x"]), p["q"], tol=tol["acq"])

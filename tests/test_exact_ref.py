"""CPU tests of tests/exact_ref.py: the extended-precision reference pinned against mpmath at 256 bits,
the three CPU implementations (oracle_np, cpu_ref.c, the grid-convolution mirror) held to the bound
the device is held to -- at cond 12, 1.4e8 and 3e10 -- and the bound's teeth: perturbations of the
inputs ten orders below the 1e-5 parity rule that it must reject."""

import numpy as np
import pytest

import exact_ref as X
import gridconv_model as G
from oracle import oracle_np as O

U = X.U
_REF = {}


def _ref(name):
    """(problem, shape, lo, grid points, exact reference over every grid point), once per case."""
    if name not in _REF:
        d, shape, lo = X.lattice_case(name)
        pts = G.grid_points(shape, lo)[::X.SUBSAMPLE]
        ref = X.exact_predict(d["x"], d["y"], d["Kinv"], d["pm"], d["pv"], d["ls"], d["betas"], pts)
        _REF[name] = (d, shape, lo, pts, ref)
    return _REF[name]


def _six_d():
    """6-D, non-integer coordinates in [0, 300)^6, N = 50, ls = 60."""
    rng = np.random.default_rng(66)
    x = rng.uniform(0, 300, size=(50, 6))
    y = rng.normal(size=(50, 2)) * 30 + 5
    d = X.relength(dict(x=x, y=y, pm=y.mean(0), pv=y.var(0), betas=np.array([1.0, 2.0])), (60.0, 60.0))
    pts = np.concatenate([x[:2], x[2:4] + rng.normal(size=(2, 6)), rng.uniform(0, 300, size=(4, 6))])
    return d, pts


def test_path_constants_stay_under_the_cap():
    for path in ("chunk-major", "gridconv"):
        for n, cols, dim in [(1, 20, 2), (40, 50, 2), (130, 64, 2), (300, 96, 2), (1700, 16, 8), (4096, 32768, 2)]:
            cq, cmu = X.path_constants(path, n, cols, dim)
            assert max(cq, cmu) <= 2 * max(n, cols) + 2 * dim + 64
            assert min(cq, cmu) >= (2 * n if path == "chunk-major" else 2 * min(n, cols))


@pytest.mark.parametrize("name", ["a", "b", "c", "6d"])
def test_reference_against_mpmath_256(name):
    """The reference's own error in q and in mu - pm, before any rounding to f64, is at most 1/8 of
    u S_q and u S_mu (a condition, not a measurement; measured <= 0.001 at N <= 130)."""
    import mpmath as mp
    if name == "6d":
        d, pts = _six_d()
    else:
        d, shape, lo = X.lattice_case(name)
        all_pts = G.grid_points(shape, lo)
        rng = np.random.default_rng(3)
        near = d["x"][:2].astype(np.int64) + np.array([[0, 1], [1, 1]])
        pts = np.concatenate([d["x"][:2].astype(np.int64), near, all_pts[rng.choice(len(all_pts), 4, replace=False)]])
    assert pts.shape[0] >= 6
    ref = X.exact_predict(d["x"], d["y"], d["Kinv"], d["pm"], d["pv"], d["ls"], d["betas"], pts)
    worst_q = worst_m = 0.0
    for o in range(len(d["pm"])):
        mm, qq = X._mp_rows(d["x"], d["y"][:, o], d["Kinv"][o], d["pm"][o], d["pv"][o], d["ls"][o], pts, 256)
        m_hi, m_lo = X.split_ld(ref["m_ext"][o])
        q_hi, q_lo = X.split_ld(ref["q_ext"][o])
        with mp.workprec(256):
            for i in range(pts.shape[0]):
                eq = abs(mp.mpf(float(q_hi[i])) + mp.mpf(float(q_lo[i])) - qq[i])
                em = abs(mp.mpf(float(m_hi[i])) + mp.mpf(float(m_lo[i])) - mm[i])
                worst_q = max(worst_q, float(eq / (U * ref["S_q"][o, i])))
                worst_m = max(worst_m, float(em / (U * ref["S_mu"][o, i])))
    print(f"{name}: cond {d['cond']:.2e}; reference error / (u S): q {worst_q:.2e}, mu {worst_m:.2e}")
    assert worst_q <= 0.125 and worst_m <= 0.125, (worst_q, worst_m)


def _implementations(d, shape, lo, pts):
    from oracle import cpu_ref
    args = (d["pm"], d["pv"], d["ls"], d["betas"])
    o = O.predict_acquire(d["x"], d["y"], pts, *args, kinv=d["Kinv"])
    yield "oracle_np", "chunk-major", {k: o[k] for k in X.OUTPUTS}
    yield "cpu_ref", "chunk-major", cpu_ref.predict_acquire(d["x"], d["y"], pts.astype(np.float64), d["Kinv"],
                                                           *args, ucb=True)
    m = G.model_predict(d["x"], d["y"], d["Kinv"], *args, shape, lo)
    yield "model_predict", "gridconv", {k: v[..., ::X.SUBSAMPLE] for k, v in m.items()}


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_cpu_implementations_meet_the_device_bound(name):
    d, shape, lo, pts, ref = _ref(name)
    for who, path, got in _implementations(d, shape, lo, pts):
        cq, cmu = X.path_constants(path, d["x"].shape[0], shape[1], 2)
        X.check_exact(got, ref, d["pv"], d["betas"], cq, cmu, f"{who} [{name}, cond {d['cond']:.1e}]")


def _perturbed(d, what):
    if what == "ls":
        return dict(d, ls=d["ls"] * (1 + 1e-11))
    if what == "kinv":
        kinv = d["Kinv"].copy()
        for o in range(kinv.shape[0]):
            kinv[o, 3, 3] *= 1 + 1e-10
        return dict(d, Kinv=kinv)
    x = d["x"].copy()
    x[3, 1] += 1e-9
    assert x[3, 1] != d["x"][3, 1]
    return dict(d, x=x)


@pytest.mark.parametrize("what", ["ls", "kinv", "coordinate"])
def test_bound_has_teeth(what):
    """The oracle on an input perturbed in the 10th or 11th digit fails the bound (case a; the 1e-5
    rule passes all three)."""
    from parity import check_predict
    d, shape, lo, pts, ref = _ref("a")
    p = _perturbed(d, what)
    o = O.predict_acquire(p["x"], p["y"], pts, p["pm"], p["pv"], p["ls"], p["betas"], kinv=p["Kinv"])
    got = {k: o[k] for k in X.OUTPUTS}
    check_predict(got, ref, d["pv"])
    cq, cmu = X.path_constants("chunk-major", d["x"].shape[0], shape[1], 2)
    with pytest.raises(AssertionError, match="beyond the bound"):
        X.check_exact(got, ref, d["pv"], d["betas"], cq, cmu, f"perturbed {what}")
    # and each of mu's and var's own bounds is broken, not only a derived output's
    tol = X.tolerances(ref, d["pv"], d["betas"], cq, cmu)
    assert (np.abs(got["var"] - ref["var"]) > tol["var"]).any()
    assert (np.abs(got["mu"] - ref["mu"]) > tol["mu"]).any()

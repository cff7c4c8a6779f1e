"""tests/exact_fit_ref.py on the CPU: the long-double references pinned against mpmath at 256 bits, the
LAPACK oracles and the numpy restatement of the blocked schedule under the hard bound on every case of
tests/test_gpu_fit_exact.py (the source of R), the checker's sensitivity (the reference's own value with
one input perturbed must fail the tight rule, unperturbed it must pass), and the edges."""

import numpy as np
import pytest

import exact_fit_ref as F
import test_fit_blocking_model as B
from exact_ref import LD, U
from oracle import oracle_np as O

mp = pytest.importorskip("mpmath")
PIN = 2.0 ** -8                     # the reference's own error, in units of u S (of u alpha |x_j|_1)


def _pin_problem(target):
    p = F.problem(48, 2, 7)
    return p, F._ls_for_cond(p["x"], 1.0, 1e-8, target)


@pytest.mark.parametrize("target", [2.0, 1e5, 1e9], ids=["cond2", "cond1e5", "cond1e9"])
def test_reference_pinned_against_mpmath(target):
    p, ls = _pin_problem(target)
    x, y, pm = p["x"], p["y"][:, 0], p["pm"][0]
    ref = F.exact_mll(x, y, pm, ls, 1e-8)
    assert target <= ref["cond"] < 40 * target
    with mp.workprec(256):
        m256 = F._mll_mp(x, y, pm, ls, 1e-8, 256)[0]
        own = float(abs(mp.mpf(ref["hi"]) + mp.mpf(ref["lo"]) - m256)) / (U * ref["S"])
    # the inverse of the same points: K = pv E, jitter 1e-6, LAPACK's X
    km = np.zeros((1, 48, 48))
    O.update_k(km, x, 0, 48, p["pv"][:1], np.array([ls]))
    X = O.invert_k(48, km)[0]
    cols = F.sample_cols(48)
    r_ld = F.exact_residual(km[0], X, 1e-6, cols)
    r_mp = F.exact_residual(km[0], X, 1e-6, cols, bits=256)
    d_rho = float(np.abs(r_ld["rho"] - r_mp["rho"]).max())
    d_left = float(np.abs(r_ld["left"] - r_mp["left"]).max())
    print(f"cond {ref['cond']:.1e}: the MLL reference's own error {own:.2e} u S; rho's {d_rho:.2e}, "
          f"the left ratio's {d_left:.2e} (max rho {r_mp['rho'].max():.3g}, left {r_mp['left'].max():.3g})")
    assert own <= PIN
    assert d_rho <= PIN and d_left <= PIN * max(1.0, float(r_mp["left"].max()))


@pytest.mark.parametrize("edge", ["std0", "pm"])
def test_edges_pinned_against_mpmath(edge):
    """std(y - pm) = 0 leaves D unscaled; a prior mean that is not mean(y)."""
    c = F.mll_case((33, 1e-8, edge))
    for o in range(3):
        ref = c["refs"][o]
        assert (ref["s2"] == 0.0) == (edge == "std0")
        with mp.workprec(256):
            m256, D, _, _, s2 = F._mll_mp(c["x"], c["y"][:, o], c["pm"][o], c["ls"][o], 1e-8, 256)
            assert (s2 == 0) == (edge == "std0")
            assert float(abs(mp.mpf(ref["hi"]) + mp.mpf(ref["lo"]) - m256)) <= PIN * U * ref["S"]
            assert float(D) == pytest.approx(ref["D"], rel=1e-12, abs=1e-300)
    if edge == "std0":                         # r = 2, -2, 0: D = r^T A^-1 r itself, 0 for r = 0
        d = c["x"][:, None, :] - c["x"][None, :, :]
        a0 = np.exp(-0.5 * np.einsum("ijd,ijd->ij", d, d) / c["ls"][0] ** 2) + 1e-8 * np.eye(33)
        assert c["refs"][0]["D"] == pytest.approx(4.0 * np.linalg.inv(a0).sum(), rel=1e-9)
        assert c["refs"][0]["D"] > 1.0 and c["refs"][2]["D"] == 0.0
    else:
        plain = F.mll_case((33, 1e-8, ""))
        assert all(c["refs"][o]["mll"] != plain["refs"][o]["mll"] for o in range(3))


def test_n1_closed_form():
    c = F.mll_case((1, 1e-8, ""))
    for o in range(3):
        ref, r = c["refs"][o], LD(c["y"][0, o]) - LD(c["pm"][o])
        a = LD(1) + LD(1e-8)
        want = -(r * r / a) / 2 - np.log(a) / 2 - F.LOG_2PI / 2
        assert ref["s2"] == 0.0 and ref["cond"] == 1.0
        assert float(abs((LD(ref["hi"]) + LD(ref["lo"])) - want)) <= PIN * U * ref["S"]


def test_not_pd_is_nan():
    """l so large that every E_ij is 1 in any precision used here, jitter 0: the second pivot is 0."""
    p = F.problem(33, 2, 3)
    ref = F.exact_mll(p["x"], p["y"][:, 0], p["pm"][0], 1e25, 0.0)
    assert np.isnan(ref["mll"])
    with pytest.raises(AssertionError):
        F.check_mll(0.0, ref, F.fit_constants("mll", 33, 2), 1.0)


# ---- the oracles under the bound: the source of R

@pytest.mark.parametrize("key", F.MLL_CASES, ids=[f"n{n}-jit{j:g}{'-' + e if e else ''}" for n, j, e in F.MLL_CASES])
def test_oracle_mll_under_the_bound(key):
    c = F.mll_case(key)
    consts = F.fit_constants("oracle", c["n"], c["dim"])
    for o in range(3):
        ref = c["refs"][o]
        if c["n"] >= 100 and not key[2] and key[1] == 1e-8:
            assert ref["cond"] < 1e3 if o == 0 else ref["cond"] >= 1e8 if o == 2 else True, (o, ref["cond"])
        F.check_mll(c["oracle"][o], ref, consts, F.mll_R(), f"oracle_np.compute_mll {key} obj {o} ls {c['ls'][o]:.4g}")
    print(f"R (MLL) = {F.mll_R():.3g}")


@pytest.mark.parametrize("name", list(F.INV_CASES))
def test_oracle_inverse_under_the_bound(name):
    c = F.inv_case(name)
    for o in range(c["n_obj"]):
        F.check_inverse(c["oracle_res"][o], F.fit_constants("inv-lu", c["n"]), c["growth"][o], F.inv_R(),
                        f"LAPACK {name} obj {o} cond1 {c['cond'][o]:.1e}")
    print(f"R (inverse) = {F.inv_R():.3g}")


@pytest.mark.parametrize("defer", [False, True], ids=["rank32", "rank64"])
@pytest.mark.parametrize("key", [k for k in F.MLL_CASES if k[0] <= 100 and k[1] == 1e-8],
                         ids=lambda k: f"n{k[0]}{'-' + k[2] if k[2] else ''}")
def test_blocked_schedule_mll_under_the_bound(key, defer):
    """tests/test_fit_blocking_model.py's numpy restatement of the device's schedule (32-column blocks, the
    rank-32 and the deferred rank-64 trailing update), finished as bo_compute_mll_each_jitter does."""
    c = F.mll_case(key)
    n = c["n"]
    for o in range(3):
        d = c["x"][:, None, :] - c["x"][None, :, :]
        E = np.exp(-0.5 * np.einsum("ijd,ijd->ij", d, d) / (c["ls"][o] * c["ls"][o]))
        yc = c["y"][:, o] - c["pm"][o]
        A, np_ = B.build(E, n, 32, False, key[1], yc)
        assert B.fit_schedule(A, n, 32, False, defer)
        var = np.var(yc)
        fit = float(np.sum(A[np_, :np_] ** 2))
        got = -0.5 * (fit / var if np.sqrt(var) > 0.0 else fit) - np.sum(np.log(np.diag(A)[:n])) - 0.5 * n * np.log(2 * np.pi)
        F.check_mll(got, c["refs"][o], F.fit_constants("mll", n, c["dim"]), F.mll_R(), f"blocked model {key} obj {o}")


@pytest.mark.parametrize("name", ["chol-n2", "chol-n33", "chol-n65"])
def test_blocked_schedule_inverse_under_the_bound(name):
    """The restated augmented Cholesky, then the Newton step X + X (I - A X) of inv_finish."""
    c = F.inv_case(name)
    n = c["n"]
    for o in range(c["n_obj"]):
        A, np_ = B.build(c["km"][o], n, 32, True, c["jitter"])
        assert B.fit_schedule(A, n, 32, True)
        x0 = -np.tril(A[np_:np_ + n, np_:np_ + n])
        x0 = x0 + np.tril(x0, -1).T
        a = c["km"][o] + c["jitter"] * np.eye(n)
        x1 = x0 + x0 @ (np.eye(n) - a @ x0)
        F.check_inverse(F.exact_residual(c["km"][o], x1, c["jitter"], c["cols"]), F.fit_constants(F.inv_path(name), n),
                        1.0, F.inv_R(), f"blocked model + Newton {name} obj {o}")


# ---- sensitivity: the reference's own value with one input perturbed

def _mll_with(c, o, ls=None, jitter=None):
    return F.exact_mll(c["x"], c["y"][:, o], c["pm"][o], c["ls"][o] if ls is None else ls,
                       c["jitter"] if jitter is None else jitter)["mll"]


def test_checker_rejects_a_length_scale_off_by_1e_11():
    c = F.mll_case((100, 1e-8, ""))
    ref = c["refs"][0]
    assert ref["cond"] < 1e3
    consts = F.fit_constants("mll", 100, 2)
    F.check_mll(ref["mll"], ref, consts, F.mll_R(), "unperturbed")
    bad = _mll_with(c, 0, ls=c["ls"][0] * (1 + 1e-11))
    print(f"l (1 + 1e-11): {F.mll_ratio(bad, ref):.3g} u S against 8 R = {8 * F.mll_R():.3g}")
    assert F.mll_ratio(bad, ref) > 8 * F.mll_R()
    with pytest.raises(AssertionError):
        F.check_mll(bad, ref, consts, F.mll_R(), "l (1 + 1e-11)")


def test_checker_rejects_a_jitter_off_by_1e_6():
    """At cond > 1e9 the checker sees jitter (1 + 1e-6) -- 1e-14 on a unit diagonal, 90 u -- only where
    tr(A^-1) is not small beside sum |A^-1_ij| and the data term: the move is 45 |tr(A^-1) - |w|^2 / s^2| u.
    Here (300 uniform points of [0, 300)^2, a noise-free toy objective, l = 200, cond 2e10) it is 3.3 u S,
    outside 8 R.  On the objectives with cond > 1e9 of the GPU module's own cases it is 0.01 - 0.9 u S
    (inside the rounding scale: no check of this kind can see it there) and 3 - 20 u S at cond < 1e3."""
    rng = np.random.default_rng(5)
    rng.uniform(0, 300, size=(300, 5))
    x = rng.uniform(0, 300, size=(300, 2))
    y = -((x[:, 0] - 40.0) ** 2) / 50.0
    ref = F.exact_mll(x, y, y.mean(), 200.0, 1e-8)
    assert ref["cond"] > 1e9
    consts = F.fit_constants("mll", 300, 2)
    F.check_mll(ref["mll"], ref, consts, F.mll_R(), "unperturbed")
    bad = F.exact_mll(x, y, y.mean(), 200.0, 1e-8 * (1 + 1e-6))["mll"]
    print(f"jitter (1 + 1e-6): moves the value by {abs(bad - ref['mll']):.3g}, {F.mll_ratio(bad, ref):.3g} u S "
          f"against 8 R = {8 * F.mll_R():.3g}")
    assert F.mll_ratio(bad, ref) > 8 * F.mll_R()
    with pytest.raises(AssertionError):
        F.check_mll(bad, ref, consts, F.mll_R(), "jitter (1 + 1e-6)")
    c = F.mll_case((65, 1e-8, ""))                 # and a well-conditioned objective of the GPU module
    assert c["refs"][0]["cond"] < 1e3
    assert F.mll_ratio(_mll_with(c, 0, jitter=1e-8 * (1 + 1e-6)), c["refs"][0]) > 8 * F.mll_R()


def test_checker_rejects_one_entry_of_the_inverse_off_by_1e_13():
    name = "chol-n257"
    c = F.inv_case(name)
    X = c["oracle"][0].copy()                  # cond 1e3: a column's diagonal entry carries a third of |x_j|_1
    cols = c["cols"]
    c_inv = F.fit_constants(F.inv_path(name), c["n"])
    F.check_inverse(F.exact_residual(c["km"][0], X, c["jitter"], cols, left=False), c_inv, 1.0, F.inv_R(), "unperturbed")
    j = int(cols[np.argmin(np.abs(X[:, cols]).sum(0))])          # the sampled column with the smallest |x_j|_1
    X[j, j] *= 1 + 1e-13
    res = F.exact_residual(c["km"][0], X, c["jitter"], cols, left=False)
    assert res["rho"].max() > 8 * F.inv_R()
    with pytest.raises(AssertionError):
        F.check_inverse(res, c_inv, 1.0, F.inv_R(), f"X[{j}, {j}] (1 + 1e-13)")


def test_sampled_columns():
    for n in (1, 33, 48, 49, 257, 2049):
        cols = F.sample_cols(n)
        assert cols.size == min(n, 48) == np.unique(cols).size and cols[0] == 0 and cols[-1] == n - 1
        assert n <= 48 or any(c % 32 == 0 for c in cols[1:]) and any(c % 32 == 31 for c in cols)
    assert np.array_equal(F.sample_cols(2049), F.sample_cols(2049))

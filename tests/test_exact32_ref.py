"""CPU tests of tests/exact32_ref.py: the counted constants stay under their cap; the numpy float32
restatement of the fp32 kernel's specified numerics meets the counted bound on every case that
tests/test_gpu_fp32_exact.py runs (its ratios, printed, are the R of the tight rule); the counted
tolerance of std_var is not vacuous on any case; and the two rules' teeth: the restatement fed perturbed
inputs -- l (1 + 1e-5), one K^-1 entry off by 1e-4, one diagonal entry of W not halved, one coordinate
moved by 1e-4 l -- is rejected."""

import numpy as np
import pytest

import exact32_ref as E

MUTANT_CASES = ("peel-n17", "peel-n65", "dim3-f64", "dim7-i64", "dim8-f64")


def test_constants_stay_under_the_cap():
    for n, dim, pv in [(1, 2, [4.0]), (65, 2, [900.0, 1500.0]), (130, 7, [1.0]), (2049, 2, [1e-5, 1e5]), (4096, 8, [2048.0])]:
        cq, cmu = E.path_constants32(n, dim, pv)
        cap = 2 * n + 2 * dim + 64
        assert (cq <= cap).all() and (cmu <= cap).all()
        assert (cq >= 2 * n).all() and (cmu >= n).all()
    with pytest.raises(AssertionError):
        E.path_constants32(10, 2, [1e9])          # |ln pv| beyond what the cap leaves room for


@pytest.mark.parametrize("name", E.CASE_NAMES)
def test_restatement_meets_the_counted_bound(name):
    d = E.case(name)
    n, dim = d["x"].shape
    rat, tol = E.check_exact32(d["restated"], d["ref"], d["sc"], d["pv"], d["betas"], n, dim,
                               f"restatement {name} (N {n}, dim {dim}, {'integer' if d['integer'] else 'non-integer'})")
    # the condition on the reference alone: std_var lives in [0, 1], a larger tolerance is vacuous
    worst = float(tol["std_var"].max())
    print(f"    tol_std_var <= {worst:.3g}; u32 S_q / pv <= {float((E.U32 * d['sc']['S_q'] / d['pv'][:, None]).max()):.3g}")
    assert worst <= 0.1, (name, worst)


def test_classes_and_R():
    """Grids and i64 sets are the integer class (c = 0 exactly: S_q is then exact_ref's with |sym A|), the f64
    and Sobol sets are not; R_var and R_mu per class."""
    for name in E.CASE_NAMES:
        d = E.case(name)
        assert d["integer"] == (d["cand"][0] in ("grid", "i64")), name
    d = E.case("dim3-f64")
    as_int = E.scales32(np.rint(d["x"]), d["y"], d["Kinv"], d["pm"], d["pv"], d["ls"], np.rint(d["pts"]))
    assert as_int["integer"]
    assert not E.integer_class(d["x"], d["pts"])
    assert not E.integer_class(np.array([[0.0, 0.0], [2.0 ** 24, 1.0]]), np.array([[1.0, 1.0]]))
    R = {(c, k): E.tight_R(c, k) for c in (True, False) for k in ("var", "mu")}
    print("R: " + ", ".join(f"{'integer' if c else 'non-integer'} {k} {v:.3g}" for (c, k), v in R.items()))
    assert all(0.1 < v < 64 for v in R.values())        # a restatement of order-one ratios, else it is broken


def test_float32_floor_is_active_at_some_candidates_only():
    d = E.case("floor32-n49")
    assert d["min_var"] == 1e-6
    floored = d["ref"]["var"] <= 1e-6
    assert floored.any() and (~floored).any(), (int(floored.sum()), floored.size)
    assert np.all(d["ref"]["var"][floored] == 1e-6)


def test_f32_range_needs_no_term_beside_2_u64_pv():
    """N = 1: far candidates have q below the f32 range; the restatement returns var = pv exactly there, many
    times u32 S_q away from the reference and far inside 2 u64 pv; T_range stays below 2^-60 of it."""
    d = E.case("peel-n1")
    ref, sc, pv = d["ref"], d["sc"], d["pv"][:, None]
    q = np.asarray(ref["q_ext"], dtype=np.float64)
    lost = (d["restated"]["var"] == pv) & (q > 0) & (q < 2.0 ** -126)
    assert lost.any()
    assert np.max(q[lost] / (E.U32 * sc["S_q"][lost])) > 1e3
    assert np.all(q[lost] <= 2.0 ** -60 * E.U64 * np.broadcast_to(pv, q.shape)[lost])
    for name in E.CASE_NAMES:
        c = E.case(name)
        assert np.all(c["sc"]["T_q"] <= 2.0 ** -60 * 2 * E.U64 * c["pv"][:, None]), name
        assert np.all(c["sc"]["T_mu"] - c["sc"]["T_alpha"] <= 2.0 ** -60 * E.U64 * np.sqrt(c["pv"])[:, None]), name
        # T_alpha (the f64 chain behind alpha: |A| |r| against |A r|) grows with cond(K); nothing else holds
        # it down, so it must stay a small fraction of the f32 term it stands beside
        frac = float(np.max(c["sc"]["T_alpha"] / (E.U32 * c["sc"]["S_mu"])))
        print(f"{name}: T_alpha / (u32 S_mu) <= {frac:.3g}")
        assert frac <= 2.0 ** -10, (name, frac)


# ---- the teeth

def _mutant(name, half=None, **changed):
    """The restatement on the case with perturbed inputs against the case's own reference: the worst var / mu
    unit ratio over 8 R, and the worst var / mu error over the counted bound."""
    d = E.case(name)
    p = dict({k: d[k] for k in ("x", "y", "Kinv", "pm", "pv", "ls", "betas")}, **changed)
    got = E.restate32(p["x"], p["y"], p["Kinv"], p["pm"], p["pv"], p["ls"], p["betas"], d["pts"],
                      min_var=d["min_var"], drop_half_row=half)
    rat = E.unit_ratios(got, d["ref"], d["sc"], d["pv"], d["betas"])
    n, dim = d["x"].shape
    tol = E.tolerances32(d["ref"], d["sc"], d["pv"], d["betas"], *E.path_constants32(n, dim, d["pv"]))
    counted = max(float(np.max(np.abs(got[k] - d["ref"][k]) / tol[k])) for k in ("var", "mu"))
    return max(rat[k] / (E.TIGHT * E.tight_R(d["integer"], k)) for k in ("var", "mu")), counted


def _near_pair(x):
    dist = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1) + 1e300 * np.eye(x.shape[0])
    return np.unravel_index(np.argmin(dist), dist.shape)


def _report(what, res):
    print(f"{what}: " + "; ".join(f"{nm} {t:.3g} x 8R, {c:.3g} x counted" for nm, (t, c) in res.items()))


def test_rejects_a_length_scale_off_by_1e_5():
    res = {nm: _mutant(nm, ls=E.case(nm)["ls"] * (1 + 1e-5)) for nm in MUTANT_CASES}
    _report("l (1 + 1e-5)", res)
    assert all(t > 1 for t, _ in res.values())          # the tight rule, on every one of these cases
    assert res["peel-n17"][1] > 1                       # and the counted bound where N is small


def test_rejects_one_kinv_entry_off_by_1e_4():
    res = {}
    for nm in MUTANT_CASES:
        d = E.case(nm)
        i, j = _near_pair(d["x"])
        A = d["Kinv"].copy()
        A[:, i, j] *= 1 + 1e-4
        res[nm] = _mutant(nm, Kinv=A)
    _report("K^-1[i, j] (1 + 1e-4), (i, j) the nearest pair", res)
    assert sum(t > 1 for t, _ in res.values()) >= 1
    assert res["peel-n17"][0] > 1


def test_rejects_a_diagonal_entry_not_halved():
    res = {nm: _mutant(nm, half=E.case(nm)["x"].shape[0] // 2) for nm in MUTANT_CASES}
    _report("W[r, r] not halved", res)
    assert all(t > 1 and c > 1 for t, c in res.values())            # both rules, every case


def test_rejects_one_coordinate_moved_by_1e_4_l():
    res = {}
    for nm in MUTANT_CASES:
        d = E.case(nm)
        x = d["x"].copy()
        x[x.shape[0] // 2, 0] += 1e-4 * d["ls"].min()
        res[nm] = _mutant(nm, x=x)
    _report("x[r, 0] + 1e-4 l", res)
    assert sum(t > 1 for t, _ in res.values()) >= 1
    assert res["peel-n17"][0] > 1 and res["peel-n17"][1] > 1

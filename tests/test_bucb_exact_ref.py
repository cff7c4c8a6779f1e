"""tests/bucb_exact_ref.py pinned on the CPU (no GPU, no library):

1. the staged formulation composed from scratch in extended precision reproduces the posterior variance
   of the GP on X u {picks} from the augmented Gram matrix (bucb_ref.posterior's formulation) evaluated
   in the same extended precision;
2. a numpy f64 emulation of the device recursion, in the device's order of operations, meets every
   stage's counted bound at cond(K + jitter I) of about 1e2, 1e8 and 1e15;
3. six subtly wrong variants of that emulation each miss the bound of the stage they belong to -- the
   evidence that tests/test_gpu_bucb_exact.py would notice such a kernel;
4. the mpmath fallback of the reference agrees with the long-double one.
"""
import functools

import numpy as np
import pytest

import bucb_exact_ref as X


def random_problem(n, dim, n_obj, m, ls, seed, kinv_jitter=None, box=60.0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, box, (n, dim))
    pts = rng.uniform(0.0, box, (m, dim))
    return X.problem(x, pts, n_obj, ls, seed, kinv_jitter=kinv_jitter)


@functools.lru_cache(maxsize=None)
def emulated(name):
    """(problem, states, vars) of the named case with the unmutated emulation, q = 6."""
    args = {"cond1e2": (120, 2, 2, 80, 3.0, 1), "cond1e8": (200, 2, 2, 80, 12.0, 2),
            "cond1e15": (200, 2, 2, 80, 12.0, 2, 1e-13), "dim8": (300, 8, 8, 40, 70.0, 3)}[name]
    pb = random_problem(*args)
    states, out = X.emulate(pb, 6)
    return pb, states, out


def worst_of(pb, states):
    worst, prev = {}, pb["var"]
    for st in states:
        X.merge(worst, X.check_step(pb, st, prev))
        prev = st["var"]
    return worst


# ---------------------------------------------------------------------------------------- 1.
def test_staged_formulation_is_the_augmented_posterior():
    """N = 20, q = 4, two objectives, cond ~ 1e2.  Both sides invert in extended precision: a Cholesky
    inverse of an n x n matrix errs by about n eps cond relative to |inv|, which the quadratic form
    turns into n eps cond S with S = pv + sum |k_i| |inv_ij| |k_j|, the reference's own cancellation
    scale; two formulations, and as much again for the products and sums: 4 (N + q) eps cond S."""
    E = X.EXT
    pb = random_problem(20, 2, 2, 50, 4.0, 5)
    assert 10 < pb["cond"] < 1e4, pb["cond"]
    xc, cc = X.centre(pb["x"], pb["pts"])
    picks = [7, 31, 2, 44]
    with E.prec():
        for o in range(2):
            var0, _ = X.augmented(E, xc, cc, [], pb["pv"][o], pb["ls"][o], pb["jitter"])
            got = X.compose(E, xc, cc, picks, pb["pv"][o], pb["ls"][o], pb["jitter"], var0)
            for t in range(4):
                want, scale = X.augmented(E, xc, cc, picks[:t + 1], pb["pv"][o], pb["ls"][o], pb["jitter"])
                err = E.f64(abs(got[t] - want))
                tol = 4 * 24 * E.eps * pb["cond"] * E.f64(scale)
                print(f"objective {o} pick {t}: worst err / tol {np.max(err / tol):.3g}, "
                      f"err / S {np.max(err / E.f64(scale)):.3g}")
                assert np.all(err <= tol)
                # the update is not a no-op: the variance at the pick fell to about the jitter
                assert float(want[picks[t]]) < 1e-5 < float(var0[picks[t]])


# ---------------------------------------------------------------------------------------- 2.
@pytest.mark.parametrize("name,lo,hi", [("cond1e2", 30, 3e3), ("cond1e8", 1e7, 1e9), ("cond1e15", 1e13, 1e17),
                                        ("dim8", 1e3, 1e9)])
def test_emulation_meets_every_bound(name, lo, hi):
    pb, states, _ = emulated(name)
    print(f"{name}: cond {pb['cond']:.3g}, picks {states[-1]['pick'].tolist()}")
    assert lo < pb["cond"] < hi, pb["cond"]
    assert len(set(states[-1]["pick"].tolist())) == 6
    worst = worst_of(pb, states)
    X.report(name, worst)
    assert set(worst) == set(X.STAGES) and all(v <= 1.0 for v in worst.values()), worst


def test_emulation_of_the_composition():
    """S7 on the emulation's own composition (the arg-max it picks by)."""
    pb, states, out = emulated("cond1e2")
    acq = (pb["std_mu"] + pb["beta"][:, None] * np.sqrt(np.abs(out[2] * (1.0 / pb["pv"])[:, None]))).sum(0)
    r = X.stage7(pb, out[2], acq)
    print("S7", r)
    assert r <= 1.0
    assert X.stage7(pb, out[2], acq * (1.0 + 1e-14)) > 1.0


# ---------------------------------------------------------------------------------------- 3.
MUTATIONS = [("drop_chunk_row", "S6", "dim8"), ("drop_pick_row", "S6", "cond1e2"), ("no_jitter", "S4", "cond1e2"),
             ("w_entry", "S2", "cond1e2"), ("u_entry", "S5", "cond1e2"), ("no_clamp", "S4", "cond1e15")]


@pytest.mark.parametrize("mut,stage,name", MUTATIONS)
def test_mutation_fails_its_stage(mut, stage, name):
    pb, states, _ = emulated(name)
    picks = states[-1]["pick"]
    if mut == "drop_chunk_row":                                # the staged chunk is full before the picks
        assert X.chunk_rows(8, 8) == 256 < pb["x"].shape[0]
    if mut == "no_clamp":                                      # the case has a negative c_tt to clamp
        neg = []
        for st in states:
            for o in range(len(pb["pv"])):
                t = st["t"]
                _, ctt, _, _, tol_d = X.coef_reference(X.EXT, st["kx"][o], st["kp"][o], st["wv"][o], st["coef"][o, :t],
                                                       st["dd"][o, :t], pb["jitter"], 1.0)
                neg.append(float(ctt) < -tol_d)
        assert any(neg), "no negative c_tt in this case"
    mstates, _ = X.emulate(pb, 6, picks=picks, mut=mut)
    worst = worst_of(pb, mstates)
    X.report(f"{mut} ({name})", worst)
    assert worst[stage] > 1.0, (mut, worst)
    # the stages take their inputs as data, so only the mutated stage fails
    assert all(v <= 1.0 for k, v in worst.items() if k != stage), worst


# ---------------------------------------------------------------------------------------- 4.
def test_mpmath_fallback_agrees():
    pb = random_problem(9, 3, 2, 12, 9.0, 8)
    states, _ = X.emulate(pb, 3)
    prev = pb["var"]
    sel = np.arange(0, 12, 4)
    for st in states:
        a = X.check_step(pb, st, prev, X._LongDouble if X.LD_OK else X._Mpmath, sel)
        b = X.check_step(pb, st, prev, X._Mpmath, sel)
        prev = st["var"]
        for k in X.STAGES:
            assert b[k] <= 1.0 and abs(a[k] - b[k]) <= 0.01 + 1e-3 * abs(a[k]), (k, a, b)


def test_constants_are_capped():
    for n, t, dim in [(1, 0, 1), (12, 47, 2), (254, 4, 8), (1362, 4, 1), (65536, 47, 8)]:
        c = X.constants(n, t, dim, [1.0])
        assert c["C_w"] == -(-n // 64) + 6 and c["C_r"] == n + t + 12 and c["C_a"] == dim + 7
    with pytest.raises(AssertionError):
        X.constants(10, 0, 2, [4.0])
    assert X.chunk_rows(1, 1) == 1364 and X.chunk_rows(8, 8) == 256 and X.chunk_rows(2, 5) == 408

"""The fit path against the extended-precision references of tests/exact_fit_ref.py: compute_mll's
per-objective terms (bo_compute_mll_each_jitter) and invert_k's per-column backward error, each under the
hard bound with its derived constants and under the 8 R rule (R: the LAPACK oracle's worst ratio over this
module's cases, computed on the CPU by exact_fit_ref.mll_R / inv_R).  The bound does not depend on the
conditioning: one call factors a well-conditioned, a middling and a fitted-regime matrix side by side
(three objectives at l near the point spacing, 4x that, and a fitted-like l), from cond 1 to 7e10 for the
MLL and past 1e16 for the inverse (the 1-norm estimate from LAPACK's own inverse: numerically singular).

Schedules and paths, each asserted from the counters: the persistent factorisation (in process), the
launch-per-step schedule at the same small N and the switch at BO_FIT_PERSIST_MAX_NBT = 2 (one child
process each: the knobs are read once per process), Cholesky + Newton in its split-k and full-k form, the
blocked LU in every panel regime and as the fallback of a failed Cholesky, Gauss-Jordan, both jitters, and
the unrefined inverse (BO_INV_REFINE=0).
Each case's reference is computed once (exact_fit_ref's cache); every test prints its ratios (pytest -s)."""

import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import exact_fit_ref as F
from bayesopt_smart_amd.config import precision_constants

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bo():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import bayesopt_smart_amd as bo
    bo._lib.load()
    return bo


def _moved(before, after):
    return {k: after[k] - before[k] for k in after}


def _case_id(key):
    n, jitter, edge = key
    return f"n{n}-jit{jitter:g}" + (f"-{edge}" if edge else "")


def _score_mll(c, terms, label):
    """Both rules on the three per-objective terms of one call; the worst ratio."""
    consts = F.fit_constants("mll", c["n"], c["dim"])
    return max(F.check_mll(terms[o], c["refs"][o], consts, F.mll_R(), f"{label} obj {o} ls {c['ls'][o]:.4g}")
               for o in range(3))


def _score_inv(c, name, got, label):
    c_inv = F.fit_constants(F.inv_path(name), c["n"])
    worst = 0.0
    for o in range(c["n_obj"]):
        res = F.exact_residual(c["km"][o], got[o], c["jitter"], c["cols"], left=c["n"] <= 1100)
        grow = 1.0 if c["path"] == "chol" else c["growth"][o]
        worst = max(worst, F.check_inverse(res, c_inv, grow, F.inv_R(),
                                           f"{label} obj {o} cond1 {c['cond'][o]:.1e} (LAPACK's rho "
                                           f"{c['oracle_res'][o]['rho'].max():.3g})"))
    return worst


# ---- the MLL on the persistent schedule

@pytest.mark.parametrize("key", F.MLL_CASES, ids=_case_id)
def test_mll_persistent(bo, key):
    import torch
    c = F.mll_case(key)
    n = c["n"]
    jitter = precision_constants(np.float32 if key[1] == 1e-4 else None)[1]
    assert jitter == key[1]
    xd, yd = torch.tensor(c["x"], device="cuda"), torch.tensor(c["y"], device="cuda")
    km = torch.zeros((3, n, n), dtype=torch.float64, device="cuda")
    before = bo._lib.fit_path_counts()
    terms = bo.kernels._mll_terms(xd, yd, km, c["pm"], c["pv"], c["ls"], n, [0, 1, 2], jitter=jitter)
    assert _moved(before, bo._lib.fit_path_counts()) == {"persistent": 1, "launches": 0, "aborted": 0}
    _score_mll(c, terms, f"MLL persistent {_case_id(key)}")


def test_mll_not_positive_definite(bo):
    """l = 1e25, jitter 0: every E_ij is 1, the second pivot 0.  The reference is NaN, the device must
    answer NaN or BO_ERR_NOT_PD."""
    import torch
    p = F.problem(33, 2, 3)
    ls = np.full(3, 1e25)
    assert np.isnan(F.exact_mll(p["x"], p["y"][:, 0], p["pm"][0], ls[0], 0.0)["mll"])
    xd, yd = torch.tensor(p["x"], device="cuda"), torch.tensor(p["y"], device="cuda")
    km = torch.zeros((3, 33, 33), dtype=torch.float64, device="cuda")
    try:
        terms = bo.kernels._mll_terms(xd, yd, km, p["pm"], p["pv"], ls, 33, [0, 1, 2], jitter=0.0)
    except np.linalg.LinAlgError:
        return
    assert all(np.isnan(terms[o]) for o in range(3)), terms


# ---- the inverse, in process

def _expected_paths(c):
    return [{"chol": 0, "lu": 1, "gj": 2}[c["path"]]] * c["n_obj"]


@pytest.mark.parametrize("name", list(F.INV_CASES))
def test_invert_k(bo, name):
    import torch
    c = F.inv_case(name)
    n, n_obj = c["n"], c["n_obj"]
    jitter = precision_constants(np.float32 if c["jitter"] == 1e-3 else None)[0]
    assert jitter == c["jitter"]
    hint = None if c["kind"] in ("chol", "asym", "fallback") else [True] * n_obj
    before = bo._lib.invert_k_path_counts(), bo._lib.fit_path_counts()
    taken = []
    got = bo.kernels.invert_k(n, torch.tensor(c["km"], device="cuda"), lu_hint=hint, paths=taken,
                              float_type=np.float32 if c["jitter"] == 1e-3 else None).cpu().numpy()
    inv_moved = _moved(before[0], bo._lib.invert_k_path_counts())
    fit_moved = _moved(before[1], bo._lib.fit_path_counts())
    assert taken == _expected_paths(c), taken
    assert inv_moved == {"cholesky": n_obj if c["path"] == "chol" else 0, "lu": n_obj if c["path"] == "lu" else 0,
                         "gauss_jordan": n_obj if c["path"] == "gj" else 0}, inv_moved
    # a factorisation ran only where the Cholesky was tried: persistent at these N, none aborted
    assert fit_moved == {"persistent": 1 if hint is None else 0, "launches": 0, "aborted": 0}, fit_moved
    _score_inv(c, name, got, f"invert_k {name} ({F.inv_path(name)})")


# ---- the schedules and knobs that are chosen once per process: one child each

CHILD = r"""
import json, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import bayesopt_smart_amd as bo
import exact_fit_ref as F
bo._lib.load()
spec = json.loads(sys.argv[3])
out, counts = {}, {}
for key in spec["mll"]:
    key = (int(key[0]), float(key[1]), key[2])
    p = F.mll_problem(key)
    n = p["n"]
    km = torch.zeros((3, n, n), dtype=torch.float64, device="cuda")
    before = bo._lib.fit_path_counts()
    t = bo.kernels._mll_terms(torch.tensor(p["x"], device="cuda"), torch.tensor(p["y"], device="cuda"), km,
                              p["pm"], p["pv"], p["ls"], n, [0, 1, 2], jitter=p["jitter"])
    after = bo._lib.fit_path_counts()
    out[f"mll_{n}"] = np.array([t[o] for o in range(3)])
    counts[f"mll_{n}"] = {k: after[k] - before[k] for k in after}
for name in spec["inv"]:
    km = F.inv_km(name)
    n = km.shape[-1]
    before = bo._lib.fit_path_counts()
    taken = []
    out[f"inv_{name}"] = bo.kernels.invert_k(n, torch.tensor(km, device="cuda"), paths=taken).cpu().numpy()
    after = bo._lib.fit_path_counts()
    counts[f"inv_{name}"] = dict({k: after[k] - before[k] for k in after}, paths=taken)
np.savez(sys.argv[2], **out)
print("COUNTS " + json.dumps(counts))
"""


def _child(env_extra, mll_keys, inv_names):
    """One fresh process with the knob set: it only runs the device and saves what it computed.  A child that
    exits with a signal or at its time limit fails the test (subprocess.run raises at the limit)."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    env = {k: v for k, v in os.environ.items() if k not in ("BO_FIT_PATH", "BO_FIT_PERSIST_MAX_NBT", "BO_INV_REFINE")}
    env.update(env_extra)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "out.npz")
        r = subprocess.run([sys.executable, "-c", CHILD, ROOT, path, json.dumps(dict(mll=mll_keys, inv=inv_names))],
                           env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (env_extra, r.returncode, r.stderr[-3000:])
        counts = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("COUNTS "))[7:])
        with np.load(path) as z:
            return {k: z[k] for k in z.files}, counts


def test_launch_per_step_schedule(bo):
    """BO_FIT_PATH=launches at N = 33 ... 513: the MLL terms and the Cholesky-path inverses of the schedule
    that otherwise runs only above N = 1536."""
    keys = [(n, 1e-8, "") for n in F.LAUNCH_NS]
    names = [f"chol-n{n}" for n in (33, 65, 257, 513)]
    out, counts = _child({"BO_FIT_PATH": "launches"}, keys, names)
    worst = 0.0
    for key in keys:
        assert counts[f"mll_{key[0]}"] == {"persistent": 0, "launches": 1, "aborted": 0}, counts
        worst = max(worst, _score_mll(F.mll_case(key), out[f"mll_{key[0]}"], f"MLL launch-per-step n{key[0]}"))
    for name in names:
        assert counts[f"inv_{name}"] == {"persistent": 0, "launches": 1, "aborted": 0, "paths": [0, 0, 0]}, counts
        _score_inv(F.inv_case(name), name, out[f"inv_{name}"], f"invert_k launch-per-step {name}")
    print(f"MLL launch-per-step: worst err / (u S) {worst:.3g}")


def test_schedule_switch_at_two_blocks(bo):
    """BO_FIT_PERSIST_MAX_NBT=2: N = 33 and 64 (two column blocks) stay persistent, N = 65 and 100 take the
    launch-per-step schedule at the boundary itself."""
    keys = [(n, 1e-8, "") for n in (33, 64, 65, 100)]
    names = ["chol-n33", "chol-n65"]
    out, counts = _child({"BO_FIT_PERSIST_MAX_NBT": "2"}, keys, names)
    for key in keys:
        sched = "persistent" if key[0] <= 64 else "launches"
        assert counts[f"mll_{key[0]}"] == dict({"persistent": 0, "launches": 0, "aborted": 0}, **{sched: 1}), counts
        _score_mll(F.mll_case(key), out[f"mll_{key[0]}"], f"MLL max_nbt=2 {sched} n{key[0]}")
    for name, sched in zip(names, ("persistent", "launches")):
        assert counts[f"inv_{name}"] == dict({"persistent": 0, "launches": 0, "aborted": 0, "paths": [0, 0, 0]},
                                             **{sched: 1}), counts
        _score_inv(F.inv_case(name), name, out[f"inv_{name}"], f"invert_k max_nbt=2 {sched} {name}")


def test_unrefined_inverse(bo):
    """BO_INV_REFINE=0 was expected to be a built-in mutant that the tight rule rejects by orders of magnitude
    (a product of triangular inverses, right residual ~ cond u).  Measured on an MI355X it is not: the
    augmented factorisation forms -K^-1 as a Schur complement, and its per-column backward error is
    rho = 3.6 / 2.5 / 9.2 at cond 1e3 / 4e8 / 5e10 (N = 257) against 2.2 / 2.0 / 1.8 with the Newton step
    and 8 R = 89.  So no rejection is asserted; the unrefined inverse is held to both rules itself, with the
    constant of the factorisation alone (c + 2: no Newton chains), and the step's effect is printed."""
    import torch
    name = "chol-n257"
    c = F.inv_case(name)
    assert 1e9 <= c["cond"][2] <= 1e12
    out, counts = _child({"BO_INV_REFINE": "0"}, [], [name])
    assert counts[f"inv_{name}"]["paths"] == [0, 0, 0]
    refined = bo.kernels.invert_k(c["n"], torch.tensor(c["km"], device="cuda")).cpu().numpy()
    assert not np.array_equal(refined, out[f"inv_{name}"])          # the knob took effect in the child
    c_chol = F.fit_constants(F.inv_path(name), c["n"]) - 2 * (4 * -(-c["n"] // 16) + 4)
    for o in range(3):
        res = F.exact_residual(c["km"][o], out[f"inv_{name}"][o], c["jitter"], c["cols"], left=False)
        ref = F.exact_residual(c["km"][o], refined[o], c["jitter"], c["cols"], left=False)
        F.check_inverse(res, c_chol, 1.0, F.inv_R(), f"BO_INV_REFINE=0 {name} obj {o} cond1 {c['cond'][o]:.1e} "
                                                     f"(with the Newton step: {ref['rho'].max():.3g})")

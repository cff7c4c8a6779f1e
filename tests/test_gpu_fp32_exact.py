"""The fp32 predict kernel (mode="fp32": cm32_predict_kernel<DIM, KQV>, pack32_range) against the
extended-precision reference of tests/exact_ref.py under the counted float32 rounding bound of
tests/exact32_ref.py:  |d var| <= Cq u32 S_q + T_abs,  |d mu| <= Cmu u32 S_mu + 2 u64 |mu| + T  (u32 = 2^-24;
the scales with their centring term, the constants counted line by line and the absolute terms are that
module's docstring).  K^-1 is data: the array handed to the device is the reference's A.

Two assertions per case, each per candidate and on all six outputs (mu, var, std_mu, std_var, ucb, acq):
the counted bound, and the tight rule -- the device's worst var and mu ratios err / (u32 S + abs) must be
<= 8 R (DESIGN §5's 8x rule), R the largest ratio that the numpy float32 restatement of the kernel's
specified numerics reaches in the same output over the cases of the same class, computed on the CPU in this
process; R_var and R_mu for the integer-coordinate cases (grids, i64 sets: the f32 casts are exact) and for the others (f64 and
Sobol sets, where the centring term is live).  No tolerance here is a number read off the device.

Cases (exact32_ref.CASE_NAMES; the smallest shapes at which each piece of structure exists, N the training
count, nch = ceil(N / 64), KQV from N mod 64):
  peel-n*     N = 1, 16, 17, 48, 49, 64, 65 on the 13 x 11 grid at (-5, 100), two objectives, all 143
              candidates scored (two full tiles and a tail of 15): KQV 1, 1, 2 -> 3, 3, 4, 4 and two chunks
              with one live k-quad;
  edge-n*     N = 1024, 1025, 1088 on a 40 x 30 grid: exactly one group of 16 E-quads, a second group of one
              chunk peeled to one k-quad, the same with a full chunk; the whole grid on the device, ~130 scored;
  groups3     N = 2049 on a 64 x 48 grid, three groups, one objective, 70 scored;
  dim*        dim 1, 3, 8 (f64), 5 (Sobol with a scale), 7 (i64): the padded dimensions, every candidate kind;
  ring-*      1 and 8 objectives at N = 81 (the W ring running on across the objectives; two live k-quads
              on the three-quad kernel), eight different l, pv and beta;
  skew-n65    a non-symmetric K^-1 (A plus a skew perturbation of 1e-3 |A|);
  floor32     float_type=np.float32: the floor 1e-6, active at the training points only.
Then: a shard bit-equal to the same slice of the whole call; the selection at topq = 5 and 17 (the two
insert routines) with the reference's own top 3 excluded; and the fallback to the f64 kernel when rows and
alpha do not fit the LDS, bit-equal to mode="auto".
Every test prints the worst err / (u32 S + abs) per output (pytest -s)."""

import numpy as np
import pytest

import exact32_ref as E
from parity import check_topq

pytestmark = pytest.mark.gpu

LDS_BYTES = 160 * 1024               # kLdsBytes, bo_predict.hip


@pytest.fixture(scope="module")
def bo():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import bayesopt_smart_amd as bo
    bo._lib.load()
    return bo


def _cands(bo, d):
    """The case's candidate set on the device; its points at the scored indices are the reference's."""
    kind = d["cand"][0]
    if kind == "grid":
        cs = bo.predict.CandidateSet.grid(d["cand"][1])
    elif kind == "sobol":
        _, dim, n, scale = d["cand"]
        cs = bo.predict.CandidateSet.sobol_set(dim, n, scale=scale)
    else:
        cs = bo.predict.CandidateSet.explicit(d["cand"][1])
    assert np.array_equal(np.asarray(cs.points(d["idx"])), d["pts"])
    return cs


def _fits_fp32(n, dim, n_obj):
    """make_plan's condition for the f32 kernel (bo_predict.hip): rows + alpha as f32 within kLdsBytes."""
    n_pad, dim_pad = -(-n // 64) * 64, dim + (dim & 1)
    return (n_pad * dim_pad + n_obj * n_pad) * 4 <= LDS_BYTES


def _call(bo, d, cs, mode="fp32", q=0, offset=0, count=None, excl=None):
    import torch
    ft = np.float32 if d["min_var"] == 1e-6 else np.float64
    res = bo.predict.predict_acquire(d["x"], d["y"], d["Kinv"], cs, d["pm"], d["pv"], d["ls"], d["betas"],
                                     outputs=E.OUTPUTS, topq=q, offset=offset, count=count, excl_points=excl,
                                     mode=mode, float_type=ft)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items() if not k.startswith("_")}


def _take(arrs, idx):
    return {k: np.asarray(arrs[k])[..., idx] for k in E.OUTPUTS}


def _check(d, got, label):
    """Both rules on the scored candidates; returns the per-candidate tolerances."""
    n, dim = d["x"].shape
    rat, tol = E.check_exact32(got, d["ref"], d["sc"], d["pv"], d["betas"], n, dim, label)
    cls = "integer" if d["integer"] else "non-integer"
    for k in ("var", "mu"):
        R = E.tight_R(d["integer"], k)
        print(f"    tight rule: {k} {rat[k]:.3g} against 8 R = {E.TIGHT * R:.3g} (R_{k} {R:.3g}, {cls} class)")
        assert rat[k] <= E.TIGHT * R, (label, "8 R rule", k, rat[k], R)
    # the f32 kernel ran: an f64 kernel (a plan that sent this shape elsewhere) would pass both rules with
    # ratios below exact32_ref.f64_ratio_ceiling, ~1e-7; f32 rounding cannot stay a thousand times that
    floor = 1e3 * E.f64_ratio_ceiling(n, dim)
    assert max(rat["var"], rat["mu"]) >= floor, (label, "no f32 rounding in the outputs", rat, floor)
    return tol


@pytest.mark.parametrize("name", E.CASE_NAMES)
def test_cases(bo, name):
    d = E.case(name)
    n, dim = d["x"].shape
    assert _fits_fp32(n, dim, len(d["pm"]))
    out = _call(bo, d, _cands(bo, d))
    _check(d, _take(out, d["idx"]), f"{name} (N {n}, dim {dim}, n_obj {len(d['pm'])}, {d['cand'][0]})")


def test_float32_floor_on_the_device(bo):
    """The floor is active at some scored candidates of the reference and inactive at others (asserted on the
    reference); the device returns nothing under 1e-6, and stays above it wherever the reference clears the
    floor by more than the counted bound."""
    d = E.case("floor32-n49")
    floored = d["ref"]["var"] <= 1e-6
    assert floored.any() and (~floored).any()
    var = _call(bo, d, _cands(bo, d))["var"][:, d["idx"]]
    tol = E.tolerances32(d["ref"], d["sc"], d["pv"], d["betas"], *E.path_constants32(*d["x"].shape, d["pv"]))["var"]
    clear = d["ref"]["var"] - tol > 1e-6
    assert clear.any() and np.all(var[clear] > 1e-6)
    assert np.all(var >= 1e-6)


@pytest.mark.parametrize("name", ["peel-n17", "peel-n65"])
def test_shard_is_bit_equal_to_the_whole_call(bo, name):
    d = E.case(name)
    cs = _cands(bo, d)
    whole = _call(bo, d, cs)
    part = _call(bo, d, cs, offset=37, count=70)
    for k in E.OUTPUTS:
        assert part[k].shape[-1] == 70
        assert np.array_equal(part[k].view(np.uint8), np.ascontiguousarray(whole[k][..., 37:107]).view(np.uint8)), k


@pytest.mark.parametrize("q", [5, 17])
def test_selection(bo, q):
    """topq = 5 (bo_wave_topq_insert16) and 17 (bo_wave_topq_insert); the evaluated points are the training
    points plus the reference's own top 3 candidates, so the exclusion probe runs on candidates that would
    otherwise win."""
    d = E.case("peel-n65")
    cs = _cands(bo, d)
    m = d["pts"].shape[0]
    assert np.array_equal(d["idx"], np.arange(m))
    is_train = np.zeros(m, dtype=bool)
    is_train[d["train_idx"]] = True
    top3 = np.argsort(-np.where(is_train, -np.inf, d["ref"]["acq"]), kind="stable")[:3]
    excluded = is_train.copy()
    excluded[top3] = True
    excl = np.concatenate([d["x"], d["pts"][top3].astype(np.float64)])
    out = _call(bo, d, cs, q=q, excl=excl)
    tol = _check(d, _take(out, d["idx"]), f"peel-n65 topq {q}")
    got = out["top_idx"]
    assert not np.isin(got[got >= 0], np.flatnonzero(excluded)).any(), got
    check_topq(got, d["ref"]["acq"], excluded, q, tol=tol["acq"])


def test_fallback_to_the_f64_kernel_is_mode_auto(bo):
    """dim 8, 8 objectives, N = 2561: (n_pad (dim_pad + n_obj)) 4 bytes exceed kLdsBytes, so make_plan leaves
    pl->fp32 unset and takes the branch that mode="auto" takes on an explicit set: every output bit-equal.
    (The K^-1 here is a diagonally dominant matrix made on the device, not an inverse: the test compares
    two runs of one kernel.)"""
    import torch
    n, dim, n_obj, m = 2561, 8, 8, 64
    assert not _fits_fp32(n, dim, n_obj) and _fits_fp32(n - 1, dim, n_obj)
    g = torch.Generator(device="cuda").manual_seed(2561)
    rng = np.random.default_rng(2561)
    x = rng.uniform(0.0, 10.0, size=(n, dim))
    y = rng.normal(size=(n, n_obj)) * 30 + 5
    pm, pv = y.mean(0), y.var(0)
    kinv = torch.rand((n_obj, n, n), generator=g, dtype=torch.float64, device="cuda") * (1e-3 / n) \
        + torch.eye(n, dtype=torch.float64, device="cuda")
    kinv /= torch.tensor(pv, device="cuda")[:, None, None]
    d = dict(x=x, y=y, Kinv=kinv, pm=pm, pv=pv, ls=np.linspace(2.0, 4.0, n_obj), betas=np.linspace(0.5, 2.5, n_obj),
             min_var=1e-10)
    cs = bo.predict.CandidateSet.explicit(np.concatenate([x[:8], rng.uniform(0.0, 10.0, size=(m - 8, dim))]))
    a = _call(bo, d, cs, mode="fp32", q=5)
    b = _call(bo, d, cs, mode="auto", q=5)
    for k in E.OUTPUTS + ("top_idx", "top_val"):
        assert np.isfinite(a[k]).all() if a[k].dtype.kind == "f" else True
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k

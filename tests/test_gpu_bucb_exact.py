"""The hallucinated-observation update on the device (bo_bucb_impl.h, as compiled into bo_select_batch_bucb,
bo_select_batch_kb and bo_select_batch_gibbon) held, stage by stage, to the counted rounding-error
bounds of tests/bucb_exact_ref.py: every stage is compared in extended precision with the device's own
outputs of the stage before it as data, so the bounds hold at any cond(K).  The independent formulation
(tests/test_gpu_bucb.py, test_gpu_kb.py, test_gpu_gibbon.py, the 1e-5 pv rule) is the complement.

Raw ABI calls: the tests own the workspace (0xFF bytes before every call, so that whatever is read was
written first) and read the update's regions back through tests/bucb_layout_model.py.  The outputs and
the inputs have ld = n_cand + 3 with NaN in the padding, kinv has ld_k = N + 5 with NaN outside the
N x N block.  kx, kp and u are overwritten at every pick, so the state after pick t comes from a run
of t + 1 picks; the picks of that run must be a prefix of the full run's.

Every test prints the worst err / tol per stage (pytest -s); DESIGN.md section 18 keeps the figures.
"""
import ctypes
import functools

import numpy as np
import pytest

import bucb_exact_ref as X
import bucb_layout_model as LM

pytestmark = pytest.mark.gpu

M = 300                 # candidates: one full and one ragged workgroup of the candidate pass
Q = 5
KINDS = ("grid", "i64", "f64", "sobol")


@pytest.fixture(scope="module")
def bo():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import bayesopt_smart_amd as bo
    return bo


# --------------------------------------------------------------------------- cases (numpy, host library)
def candidates(kind, dim, m, offset, seed):
    """(description, pts [m, dim]): the shard [offset, offset + m) of a candidate set of `kind`; pts holds
    the values the device decodes (int64 for grid / i64)."""
    from bayesopt_smart_amd.predict import CandidateSet
    rng = np.random.default_rng(seed + 77)
    idx = np.arange(offset, offset + m)
    if kind == "grid":
        side = 2
        while side ** dim < offset + m:
            side += 1
        lo = [100 + 7 * k for k in range(dim)]
        cs = CandidateSet.grid([(l, l + side + (k % 2)) for k, l in enumerate(lo)])
        return dict(kind=kind, set=cs), cs.points(idx)
    if kind == "sobol":
        cs = CandidateSet.sobol_set(dim, offset + m, lo=-2.0, scale=40.0, bits=30)
        return dict(kind=kind, set=cs), cs.points(idx)
    if kind == "i64":
        return dict(kind=kind), rng.integers(0, 61, (m, dim)).astype(np.int64)
    return dict(kind=kind), rng.uniform(0.0, 60.0, (m, dim))


def make_case(kind, dim, n_obj, n, m=M, seed=0, offset=0, ls=None, kinv_jitter=None, mask=None, cond=False):
    cand, pts = candidates(kind, dim, m, offset, seed)
    rng = np.random.default_rng(seed)
    p64 = pts.astype(np.float64)
    ext = np.maximum(np.ptp(p64, axis=0), 1.0)
    x = p64.min(axis=0) + rng.uniform(0.0, 1.0, (n, dim)) * ext
    if ls is None:                # a quarter of the diameter: the picks do not sit on one plateau
        ls = 0.25 * ext.max() * np.sqrt(dim) * (1.0 + 0.1 * np.arange(n_obj))
    pb = X.problem(x, pts, n_obj, ls, seed, kinv_jitter=kinv_jitter, want_cond=cond)
    if cond:
        print(f"cond(K + {kinv_jitter or pb['jitter']:g} I) = {pb['cond']:.3g}")
    pb.update(cand=cand, offset=offset, mask=np.zeros(m, dtype=bool) if mask is None else mask)
    return pb


# --------------------------------------------------------------------------- device side
def pack_mask(bits, words):
    out = np.zeros(words, dtype=np.uint32)
    packed = np.packbits(bits.astype(np.uint8), bitorder="little")
    out.view(np.uint8)[:packed.size] = packed
    return out


def call(entry, pb, q):
    """One call of `entry` ("bucb", "kb", "gibbon") for q picks with var_out set.  Returns the update's
    workspace regions (bucb_layout_model's names), var [n_obj, M], top_idx, top_val, acq (bucb: acq_out),
    after checking that the padding of every output is untouched."""
    import torch
    from bayesopt_smart_amd import _lib
    lib = _lib.load()
    x, pts = pb["x"], pb["pts"]
    n, dim = x.shape
    n_obj, m = len(pb["pv"]), pts.shape[0]
    ld, ld_k = m + 3, n + 5
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")  # noqa: E731

    def padded(a):                                             # [n_obj, m] -> [n_obj, ld], NaN padding
        out = np.full((a.shape[0], ld), np.nan)
        out[:, :m] = a
        return dev(out)

    kinv = np.full((n_obj, ld_k, ld_k), np.nan)
    kinv[:, :n, :n] = pb["kinv"]
    words = int(lib.bo_excl_mask_bytes(m)) // 4
    keep = dict(x=dev(x), kinv=dev(kinv), var=padded(pb["var"]), mask=dev(pack_mask(pb["mask"], words).view(np.int32)))
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")  # noqa: E731
    out = dict(top_val=nan(q), top_idx=torch.full((q,), -7, dtype=torch.int64, device="cuda"), var=nan(n_obj, ld),
               acq=nan(ld))
    d = {"bucb": _lib.BucbDesc, "kb": _lib.KbDesc, "gibbon": _lib.GibbonDesc}[entry]()
    d.n_obj, d.dim, d.n_train = n_obj, dim, n
    d.x_train, d.kinv, d.ld_k = keep["x"].data_ptr(), keep["kinv"].data_ptr(), ld_k
    d.q, d.n_cand, d.cand_offset = q, m, pb["offset"]
    kind = pb["cand"]["kind"]
    d.cand_kind = {"i64": _lib.CAND_I64, "f64": _lib.CAND_F64, "grid": _lib.CAND_GRID, "sobol": _lib.CAND_SOBOL}[kind]
    if kind == "grid":
        for k in range(dim):
            d.grid_lo[k], d.grid_shape[k] = pb["cand"]["set"].lo[k], pb["cand"]["set"].shape[k]
    elif kind == "sobol":
        d.cand = pb["cand"]["set"].cand_arg
    else:
        keep["cand"] = dev(pts)
        assert keep["cand"].dtype == (torch.int64 if kind == "i64" else torch.float64)
        d.cand = keep["cand"].data_ptr()
    for o in range(n_obj):
        d.prior_var[o], d.length_scale[o] = pb["pv"][o], pb["ls"][o]
    d.jitter, d.min_variance = pb["jitter"], pb["min_var"]
    d.var, d.ld, d.mask = keep["var"].data_ptr(), ld, keep["mask"].data_ptr()
    d.top_val, d.top_idx, d.var_out = out["top_val"].data_ptr(), out["top_idx"].data_ptr(), out["var"].data_ptr()
    if entry == "bucb":
        keep["smu"] = padded(pb["std_mu"])
        for o in range(n_obj):
            d.beta[o] = pb["beta"][o]
        d.std_mu, d.acq_out = keep["smu"].data_ptr(), out["acq"].data_ptr()
        size, run = lib.bo_select_batch_bucb_workspace_size, lib.bo_select_batch_bucb
    elif entry == "gibbon":
        keep["base"] = dev(np.concatenate([pb["base"], [np.nan] * 3]))
        d.base, d.acq_last = keep["base"].data_ptr(), out["acq"].data_ptr()
        size, run = lib.bo_select_batch_gibbon_workspace_size, lib.bo_select_batch_gibbon
    else:
        keep["mu"] = padded(pb["mu"])
        keep["front"] = np.ascontiguousarray(pb["front"], dtype=np.float64)
        out["believed"] = nan(q, n_obj)
        d.mu, d.front, d.n_front = keep["mu"].data_ptr(), keep["front"].ctypes.data, keep["front"].shape[0]
        for o in range(n_obj):
            d.ref_point[o] = -10.0
        d.form, d.box_capacity = 0, 1 << 14
        d.believed, d.acq_last = out["believed"].data_ptr(), out["acq"].data_ptr()
        size, run = lib.bo_select_batch_kb_workspace_size, lib.bo_select_batch_kb
        hbytes = lib.bo_select_batch_kb_host_workspace_size(ctypes.byref(d))
        assert hbytes > 0
        keep["host"] = torch.full((hbytes,), 0xFF, dtype=torch.uint8).pin_memory()
        d.host_ws, d.host_ws_bytes = keep["host"].data_ptr(), hbytes
    nbytes = size(ctypes.byref(d))
    lay = LM.layout(n, dim, n_obj, q, m, ld, True)
    assert nbytes == lay["total"] if entry != "kb" else nbytes >= lay["total"]
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    status = run(ctypes.byref(d), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert status == 0, status
    raw = ws.cpu().numpy()
    res = {name: LM.read(raw, lay, name) for name in LM.ORDER if name in lay}
    var = out["var"].cpu().numpy()
    acq = out["acq"].cpu().numpy()
    assert np.isnan(var[:, m:]).all() and np.isnan(acq[m:]).all(), "an output's padding was written"
    assert not np.isnan(var[:, :m]).any()
    for name, before in (("var", pb["var"]),):                 # the inputs stay as they are
        assert np.array_equal(keep[name].cpu().numpy()[:, :m], before)
    res.update(var=var[:, :m].copy(), acq=acq[:m].copy(), top_idx=out["top_idx"].cpu().numpy(),
               top_val=out["top_val"].cpu().numpy(), mask_words=(m + 31) // 32)
    return res


def stage0(pb, r, t):
    """S0, bitwise, on the run of t + 1 picks."""
    xc, cc = X.centre(pb["x"], pb["pts"])
    assert r["xc"].tobytes() == xc.tobytes(), "xc"
    want = np.where(r["top_idx"] >= 0, r["top_idx"] - pb["offset"], -1)
    np.testing.assert_array_equal(r["pick"], want)
    taken = pb["mask"].copy()
    for s, p in enumerate(r["pick"]):
        if p >= 0:
            assert 0 <= p < pb["pts"].shape[0] and not taken[p], ("a pick is masked or repeated", s, p)
            taken[p] = True
            assert r["pc"][s].tobytes() == cc[p].tobytes(), ("pc", s)
        else:
            assert not r["pc"][s].any() and np.isneginf(r["top_val"][s]) and (~taken).sum() == 0
    np.testing.assert_array_equal(r["mask"][:r["mask_words"]], pack_mask(taken, r["mask_words"]))


def run_case(entry, pb, q=Q, label=""):
    """Every stage at every pick of a batch of q; returns (worst ratios, the runs)."""
    runs = [call(entry, pb, qp) for qp in range(1, q + 1)]
    full = runs[-1]["pick"]
    worst, prev = {}, pb["var"]
    for t, r in enumerate(runs):
        np.testing.assert_array_equal(r["pick"], full[:t + 1])       # deterministic: a prefix
        stage0(pb, r, t)
        st = dict(r, t=t)
        X.merge(worst, X.check_step(pb, st, prev))
        if entry == "bucb":
            s7 = X.stage7(pb, prev, r["acq"])
            if full[t] >= 0:
                s7 = max(s7, X.stage7(pb, prev, r["top_val"][t:t + 1], [full[t]]))
            X.merge(worst, {"S7": s7})
        prev = r["var"]
    X.report(f"{entry} {label} picks {full.tolist()}", worst)
    return worst, runs


def assert_within(worst, entry):
    stages = X.STAGES + (("S7",) if entry == "bucb" else ())
    assert set(worst) == set(stages), worst
    assert all(v <= 1.0 for v in worst.values()), worst


def with_entry_inputs(pb, entry, seed=0):
    """The inputs that only one entry point reads: gibbon's `base`, kb's mu and front."""
    rng = np.random.default_rng(seed + 500)
    n_obj, m = len(pb["pv"]), pb["pts"].shape[0]
    if entry == "gibbon":
        pb["base"] = rng.standard_normal(m)
    if entry == "kb":
        pb["mu"] = np.sqrt(pb["pv"])[:, None] * pb["std_mu"]
        pb["front"] = rng.uniform(-1.0, 1.0, (3, n_obj))
    return pb


# 1. every instantiation at its chunk edge: N = RC - 2, so that the rows N + t + 1 of picks 0..4 are RC - 1,
# RC (a full chunk), then a second chunk of one, two and three rows that holds only picks
def instantiation(a, b):
    """(dim, n_obj, kind) of DIMP = 2 (a + 1), NOB = (1, 2, 3, 4, 8)[b]: odd and even dims alternate, so do
    5 and 8 objectives, and every kind occurs with every DIMP."""
    dim = 2 * a + (1 if (a + b) % 2 == 0 else 2)
    n_obj = (1, 2, 3, 4, 5 if a % 2 == 0 else 8)[b]
    return dim, n_obj, KINDS[(a + b) % 4]


def test_instantiations_cover_the_matrix():
    cells = [instantiation(a, b) for a in range(4) for b in range(5)]
    assert {d for d, _, _ in cells} == set(range(1, 9)) and {o for _, o, _ in cells} == {1, 2, 3, 4, 5, 8}
    for kind in KINDS:
        assert len({(d + 1) // 2 for d, _, k in cells if k == kind}) >= 2
    assert {((d + 1) & ~1, X.nob_of(o)) for d, o, _ in cells} == {(p, w) for p in (2, 4, 6, 8) for w in (1, 2, 3, 4, 8)}
    assert X.chunk_rows(1, 1) - 2 == 1362 and X.chunk_rows(8, 8) - 2 == 254


def edge_case(entry, dim, n_obj, kind):
    n = X.chunk_rows(dim, n_obj) - 2
    return with_entry_inputs(make_case(kind, dim, n_obj, n, seed=dim * 10 + n_obj), entry, seed=dim * 10 + n_obj)


@pytest.mark.parametrize("a,b", [(a, b) for a in range(4) for b in range(5)])
def test_bucb_every_instantiation_at_its_chunk_edge(bo, a, b):
    dim, n_obj, kind = instantiation(a, b)
    pb = edge_case("bucb", dim, n_obj, kind)
    worst, runs = run_case("bucb", pb, label=f"dim {dim} n_obj {n_obj} {kind} N {pb['x'].shape[0]}")
    assert_within(worst, "bucb")
    assert (runs[-1]["pick"] >= 0).all()


@pytest.mark.parametrize("entry,dim,n_obj,kind", [
    ("gibbon", 1, 1, "f64"), ("gibbon", 2, 8, "grid"), ("gibbon", 7, 1, "sobol"), ("gibbon", 8, 8, "i64"),
    ("kb", 2, 1, "grid"), ("kb", 1, 4, "sobol"), ("kb", 8, 1, "f64"), ("kb", 7, 4, "i64")])
def test_corners_of_the_other_entry_points(bo, entry, dim, n_obj, kind):
    pb = edge_case(entry, dim, n_obj, kind)
    worst, runs = run_case(entry, pb, label=f"dim {dim} n_obj {n_obj} {kind} N {pb['x'].shape[0]}")
    assert_within(worst, entry)
    assert (runs[-1]["pick"] >= 0).all()


# 2. small and ragged N: the mat-vec's 16-row workgroups, the 64-lane stride, a single training row
@pytest.mark.parametrize("n", [1, 15, 17, 63, 65])
def test_small_and_ragged_n(bo, n):
    pb = make_case("grid", 2, 2, n, seed=n)
    worst, _ = run_case("bucb", pb, label=f"N {n}")
    assert_within(worst, "bucb")


# 3. the largest q: s_e / s_a of the coefficient kernel and every triangular row, at every t
def test_largest_q(bo):
    pb = make_case("grid", 2, 2, 12, m=256, seed=48)
    worst, runs = run_case("bucb", pb, q=48, label="q 48")
    assert_within(worst, "bucb")
    assert len(set(runs[-1]["pick"].tolist())) == 48


# 4. conditioning: cond(K + 1e-6 I) ~ 1e8, and kinv built at jitter 1e-13 (cond ~ 1e15) with the call's 1e-6
@pytest.mark.parametrize("kinv_jitter", [None, 1e-13])
def test_conditioning(bo, kinv_jitter):
    pb = make_case("grid", 2, 2, 280, seed=3, ls=(20.0, 20.0), kinv_jitter=kinv_jitter, cond=True)
    worst, _ = run_case("bucb", pb, label=f"kinv at jitter {kinv_jitter or 1e-6:g}")
    assert_within(worst, "bucb")


# 5. a shard with a caller's mask that leaves fewer candidates than q
def test_shard_with_fewer_candidates_than_q(bo):
    mask = np.ones(M, dtype=bool)
    mask[[5, 255, 299]] = False
    pb = make_case("grid", 2, 2, 30, seed=9, offset=333, mask=mask)
    worst, runs = run_case("bucb", pb, label="shard")
    assert_within(worst, "bucb")
    full = runs[-1]
    assert sorted(full["pick"][:3].tolist()) == [5, 255, 299] and full["pick"][3:].tolist() == [-1, -1]
    assert sorted(full["top_idx"][:3].tolist()) == [338, 588, 632]
    for t in (3, 4):                                          # the steps without a pick are left out
        r = runs[t]
        assert not r["kx"].any() and not r["kp"][:, :t + 1].any() and not r["ok"].any()
        assert not r["coef"][:, t, :t + 1].any() and (r["dd"][:, t] == 1.0).all()
        assert r["var"].tobytes() == runs[t - 1]["var"].tobytes()
    assert runs[2]["ok"].all() and runs[2]["var"].tobytes() != runs[1]["var"].tobytes()


# 6. the step that is left out because d_t is not positive, made exact: kinv = 0 (it is data), pv = 1,
# jitter = 0, min_variance = 0 and two identical candidates as picks 0 and 1 give e = [1, 1], g = 1,
# c_tt = 0 and d_1 = 0 exactly
@functools.lru_cache(maxsize=None)
def left_out_problem():
    rng = np.random.default_rng(21)
    pts = rng.uniform(0.0, 60.0, (M, 2))
    i, j = 5, 200
    pts[j] = pts[i]
    x = rng.uniform(0.0, 60.0, (10, 2))
    pb = X.problem(x, pts, 2, (15.0, 18.0), 21, jitter=0.0, min_var=0.0, kinv=np.zeros((2, 10, 10)))
    pb["pv"] = np.ones(2)
    pb["var"] = np.full((2, M), 2.0)                          # data: above pv, so no variance reaches 0
    pb["std_mu"][:, [i, j]] = [[100.0, 99.0], [0.0, 0.0]]
    pb["base"] = rng.standard_normal(M)
    pb["base"][[i, j]] = [100.0, 99.0]
    pb["mu"] = rng.standard_normal((2, M))
    pb["mu"][:, i], pb["mu"][:, j] = 10.0, 9.5
    pb["front"] = np.zeros((1, 2))
    pb.update(cand=dict(kind="f64"), offset=0, mask=np.zeros(M, dtype=bool))
    return pb, i, j


@pytest.mark.parametrize("entry", ["bucb", "kb", "gibbon"])
def test_step_left_out_exactly(bo, entry):
    pb, i, j = left_out_problem()
    worst, runs = run_case(entry, pb, q=3, label="d_1 = 0")
    assert runs[2]["pick"][:2].tolist() == [i, j] and runs[2]["pick"][2] >= 0
    r = runs[1]
    assert (r["kp"][:, :2] == 1.0).all() and (runs[0]["dd"][:, 0] == 1.0).all()       # e = [1, 1], d_0 = 1
    assert not r["ok"].any(), "step 1 has d_1 = 0 and must be left out"
    assert not r["coef"][:, 1, :2].any() and (r["dd"][:, 1] == 1.0).all() and not r["u"][:, :12].any()
    assert r["var"].tobytes() == runs[0]["var"].tobytes()
    assert runs[0]["ok"].all() and runs[2]["ok"].all()
    assert (runs[0]["var"][:, [i, j]] == 1.0).all()           # 2 - k(c, c)^2 / d_0
    assert runs[2]["var"].tobytes() != r["var"].tobytes()
    assert_within(worst, entry)                               # picks 0 and 2 pass S1..S6 as usual

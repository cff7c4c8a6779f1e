"""A counted float32 rounding bound for the fp32 predict kernel (mode="fp32": cm32_predict_kernel<DIM, KQV>,
bo_predict_impl.h, fed by pack32_range and predict_prep_kernel, bo_predict.hip), a plain numpy float32
restatement of its specified numerics, and the cases the CPU and the GPU tests share.  Helper module: no
tests in it (tests/test_exact32_ref.py, tests/test_gpu_fp32_exact.py).

The reference is exact_ref.exact_predict as it stands: the f64 inputs as given, K^-1 as DATA (the array A
handed to the device), everything in long double (mpmath where long double is f64); its min_var argument
carries the float32 branch's floor.

The bound has exact_ref's shape, with u32 = 2^-24 for the f32 part and u64 = 2^-53 for the f64 part:
    |d var| <= Cq  u32 S_q  + T_abs                 T_abs = 2 u64 pv + T_range_q
    |d mu|  <= Cmu u32 S_mu + 2 u64 |mu| + T_alpha + T_range_mu
    S_q  = sum_nm (1 + a_n + a_m + c_n + c_m) k_n |sym A|_nm k_m         sym A = (A + A^T) / 2
    S_mu = sum_n  (1 + a_n + c_n) k_n |alpha_n|                          alpha = A r
a_n = |p - x_n|^2 / (2 l^2) is the exponent's argument (a relative error d of the argument is a relative
error a_n d of k_n).  alpha enters the f32 chain as ONE number per row (the cast of the f64 alpha_n), so
S_mu carries |A r|, not |A| |r|; what the f64 chain that formed alpha_n lost is T_alpha below.

The centring term c_n.  The kernel centres the coordinates on training row 0 (z) in f64 and only then
casts them to f32 (xs[t] = (float) xc[t], c32[k] = (float)(c[k] - z[k])).  The two casts leave
|d (p_k - x_nk)| <= u32 (|x_nk - z_k| + |p_k - z_k|), which is not a multiple of |p_k - x_nk|: in the
argument a_n = sum_k (p_k - x_nk)^2 / (2 l^2) that is
    c_n = sum_k |p_k - x_nk| (|x_nk - z_k| + |p_k - z_k|) / l^2          (times u32, constant 1).
exact_ref names this term for f64 and leaves it inside the chain's slack; at u32 it is carried.  It is
exactly 0 when every centred coordinate of the case (training rows and scored candidates) is an integer
below 2^24 -- every grid and i64 set near its row 0 -- because the casts are then exact; `integer_class`
decides that from the data.  On non-integer sets c_n is the bound's dominant term, as it should be: with
extent L the casts cost (L / l)(|p - x_n| / l) u32 in k_n, which is what f32 coordinates cost.

The constants, counted from the code (bayesopt_smart_amd/csrc; one unit = one relative rounding u32 of a
term k_n W_nm k_m of q, or k_n alpha_n of mu - pm):

  q = 2 k . (W k), W = f32(triu(sym A)), diagonal halved
    t = W k            acc[e][b] = mfma32(w, B, acc) (bo_predict_impl.h:1419): v_mfma_f32_16x16x4_f32 is a
                       k-ordered f32 fma chain, one rounding per product; a row's accumulator takes one
                       product per column f >= row; products with a padded row or column are exact zeros N
    k . t              qpart = fmaf(B, acc, qpart) (:1430) per lane over its rows, <= N live terms           N
                       the two adds across the lane groups, __shfl_xor 16 and 32 (:1458-1459)                2
    W                  pack32_range (bo_predict.hip:302-306): 0.5 (A_nm + A_mn) in f64, one f64 rounding
                       (2^-29 of a unit; counted 1), and the cast (float) w                                  2
    K*, twice (k_n and k_m), each:
                       v_exp_f32 (__builtin_amdgcn_exp2f, :1350): 1 ulp by the ISA, counted with 1 of slack  2
                       the rounding of the argument's fma, fmaf(d2, nl2, lpv) (:1350): absolute
                       u32 |log2 k_n|, so relative u32 |ln pv - a_n| in k_n: L = ceil |ln pv| here, 1 in
                       the a-weighted count below                                                            L
                       lpv = (float) log2(pv) (:1344): relative u32 |ln pv| in k_n                           L
                                                                                                 2 x (2 + 2L)
    the exponent's argument (a-weighted, once: S carries a_n + a_m):
                       nl2 = (float)(nhl log2 e) (:1343; nhl = -0.5 / (ls ls), bo_predict.hip:811, three
                       f64 roundings = 2^-27 of a unit): counted                                             2
                       the argument's fma, its a part                                                        1
                       d2 (:1349): the f32 difference r[k] - c32[k] enters squared, 2; one fmaf per
                       dimension, each rounding the partial sum, dim (padded dimensions hold exact zeros)
                                                                                                      dim + 2
  Cq = 2N + dim + 13 + 4L.

  mu - pm = k . (float) alpha
    the chain          mpart = fmaf(av, B, mpart) (:1404) per lane over its rows, <= N live terms            N
                       the two shuffle adds (:1460-1461)                                                     2
    alpha              al[t] = (float) a.alpha[t] (:1313)                                                    1
    K*, once           as above                                                                        2 + 2L
    the argument       as above                                                                       dim + 5
  Cmu = N + dim + 10 + 2L.

  Neither may exceed 2N + 2 dim + 64 (exact_ref's cap); path_constants32 asserts it, which bounds L by 12
  (pv between e^-12 and e^12).

  Everything after mu - pm and q is f64 (:1462-1468) and keeps exact_ref's u64 terms: 2 u64 pv for the
  subtraction pv - 2 q and the output, 2 u64 |mu| for pm + ., and exact_ref.tolerances' propagation to
  std_mu, std_var, ucb and acq (acq_bound with the per-candidate eps).

The absolute terms.
  T_alpha.  alpha_n = sum_e A_ne r_e is an f64 chain in the prep kernel (one wave per row, a shuffle tree):
  |d alpha_n| <= (N + 1) u64 (|A| |r|)_n, so T_alpha = (N + 1) u64 sum_n k_n (|A| |r|)_n.
  T_range: the f32 range.  Below eta = 2^-126 an f32 result loses bits (an absolute error of 2^-150 per
  operation where subnormals are kept) or vanishes (v_exp_f32 and a flushing mode: an absolute error below
  eta).  Taking eta per operation, whatever the mode:
    a K* entry off by eta moves q by at most 2 eta sum_m |sym A|_nm k_m, over all n:
                                                                 2 eta . 2 sum_nm |sym A|_nm k_m
    each of the <= N fmas of row n's accumulator errs by eta, times k_n:   2 eta . N sum_n k_n
    each of the <= N + 2 operations of k . t errs by eta:                  2 eta . (N + 2)
  T_range_q = 2 eta (N sum k + N + 2 + 2 sum_nm |sym A|_nm k_m); likewise for the mean, a flushed alpha_n
  and the chain's own operations, T_range_mu = eta (sum k + sum |alpha| + N + 2).
  Against the 2 u64 pv that T_abs always holds this is nothing for these cases' |W|: N sum k <= N^2 pv is
  2^33 at N = 2049 and pv = 2^11, so T_range_q is of order 2^-90 against 2^-52 pv, and tests/test_exact32_ref.py
  asserts T_range_q <= 2^-60 . 2 u64 pv on every case.  The case that shows the f32 range most --
  N = 1, l = 1.5, a candidate 17 cells away: q = pv 2^-140, where a plain f32 evaluation returns 0, 2.6e4
  times u32 S_q -- is an error of 2^-88 of 2 u64 pv.  So no term beside 2 u64 pv is NEEDED; T_range is
  carried all the same, computed from the data, so that a case with a large |W| cannot outgrow the argument
  unnoticed.  A change of the kernel that moved pv out of the exponent (k_n pv as a product) would have to
  redo this arithmetic.

The restatement (`restate32`) is the specification above in plain numpy float32: the same casts (centre in
f64, cast, subtract in f32), d2 as numpy's own f32 sum, the argument d2 nl2 + lpv in f32, np.exp2 in f32, W
as above, q = 2 k . (W k) and k . alpha as numpy's f32 products in numpy's own summation order, and the f64
tail.  Its ratios err / (u32 S + abs) at Cq = Cmu = 1 are the yardstick R of the tight rule (DESIGN §5's
8x rule, mll_grad_ref.TIGHT): the device's worst var and mu ratios must be <= 8 R, R the restatement's
largest ratio of the same output over the cases of the same class -- R_var and R_mu for the
integer-coordinate cases, R_var and R_mu for the others (tighter than one R per class: a grid case's mu is
not judged by the i64 set's var).

Where long double is no wider than f64 (exact_ref.LD_OK false: not x86) `case` scores every
exact_ref.SUBSAMPLE-th candidate only, as the f64 tests do.  The per-case bound tests adapt to that; the
selection test and the shard test of tests/test_gpu_fp32_exact.py need every candidate of their case scored
and FAIL there by their own precondition (they do not skip): on such a host run them with the mpmath
reference at SUBSAMPLE = 1.
"""

import numpy as np

import exact_ref as X
from oracle import oracle_np as O

U32 = 2.0 ** -24
U64 = X.U
ETA = 2.0 ** -126
TIGHT = 8.0                      # mll_grad_ref.TIGHT, exact_fit_ref.TIGHT: the project's 8x rule
OUTPUTS = X.OUTPUTS
F32 = np.float32


def path_constants32(n, dim, pv):
    """(Cq, Cmu) [n_obj] of the module docstring's count."""
    L = np.ceil(np.abs(np.log(np.asarray(pv, dtype=np.float64))))
    cq = 2 * n + dim + 13 + 4 * L
    cmu = n + dim + 10 + 2 * L
    cap = 2 * n + 2 * dim + 64
    assert (cq <= cap).all() and (cmu <= cap).all(), (n, dim, cq, cmu, cap)
    return cq, cmu


def integer_class(x, pts):
    """True when every coordinate centred on training row 0 is an integer below 2^24: the f32 casts are exact."""
    z = np.asarray(x, dtype=X.LD)[0]
    for v in (np.asarray(x).astype(X.LD) - z, np.asarray(pts).astype(X.LD) - z):
        if not (np.all(v == np.rint(v)) and np.all(np.abs(v) < 2.0 ** 24)):
            return False
    return True


def scales32(x, y, kinv, pm, pv, ls, pts):
    """S_q, S_mu, T_q (= T_range_q), T_mu (= T_alpha + T_range_mu), T_alpha [n_obj, M] in f64, and the class."""
    x = np.asarray(x)
    pts = np.asarray(pts)
    y = np.asarray(y, dtype=np.float64)
    n, n_obj, m = x.shape[0], len(pm), pts.shape[0]
    xl, pl = x.astype(X.LD), pts.astype(X.LD)
    dd = np.abs((pl[:, None, :] - xl[None, :, :]).astype(np.float64))          # [M, N, dim]
    sq = np.einsum("mnd,mnd->mn", dd, dd)
    integer = integer_class(x, pts)
    if integer:
        cw = np.zeros_like(sq)
    else:
        xz = np.abs((xl - xl[0]).astype(np.float64))                          # [N, dim]
        pz = np.abs((pl - xl[0]).astype(np.float64))                          # [M, dim]
        cw = np.einsum("mnd,mnd->mn", dd, xz[None, :, :] + pz[:, None, :])
    out = {k: np.empty((n_obj, m)) for k in ("S_q", "S_mu", "T_q", "T_mu", "T_alpha")}
    for o in range(n_obj):
        A = np.asarray(kinv, dtype=np.float64)[o, :n, :n]
        B = np.abs(0.5 * (A + A.T))
        r = y[:n, o] - float(pm[o])
        alpha = np.abs(A @ r)
        l2 = float(ls[o]) ** 2
        a = sq / (2.0 * l2)
        w = a + cw / l2
        k = float(pv[o]) * np.exp(-a)
        t = k @ B
        out["S_q"][o] = np.einsum("mn,mn->m", t, k) + 2.0 * np.einsum("mn,mn->m", (w * k) @ B, k)
        out["S_mu"][o] = (k * (1.0 + w)) @ alpha
        sk = k.sum(1)
        out["T_q"][o] = 2.0 * ETA * (n * sk + n + 2 + 2.0 * t.sum(1))
        out["T_alpha"][o] = (n + 1) * U64 * (k @ (np.abs(A) @ np.abs(r)))
        out["T_mu"][o] = out["T_alpha"][o] + ETA * (sk + alpha.sum() + n + 2)
    out["integer"] = integer
    return out


def tolerances32(ref, sc, pv, betas, cq, cmu):
    """Per-candidate tolerances of every output: the f32 part folded into exact_ref.tolerances' scales
    (in units of u64), so that its propagation and its u64 terms apply unchanged."""
    cq = np.broadcast_to(np.asarray(cq, dtype=np.float64), (len(pv),))[:, None]
    cmu = np.broadcast_to(np.asarray(cmu, dtype=np.float64), (len(pv),))[:, None]
    return X.tolerances(_folded(ref, sc, cq, cmu), pv, betas, 1.0, 1.0)


def _folded(ref, sc, cq, cmu):
    return dict(ref, S_q=(cq * U32 * sc["S_q"] + sc["T_q"]) / U64, S_mu=(cmu * U32 * sc["S_mu"] + sc["T_mu"]) / U64)


def unit_ratios(got, ref, sc, pv, betas):
    """Worst err / (u32 S + abs) per output at Cq = Cmu = 1: the figures of the tight rule (var, mu)."""
    return X.ratios(got, ref, tolerances32(ref, sc, pv, betas, 1.0, 1.0))


def check_exact32(got, ref, sc, pv, betas, n, dim, label=""):
    """The counted bound on every output in `got` (exact_ref.check_exact on the folded scales, which asserts
    per candidate); prints and returns the unit ratios and the tolerances."""
    cq, cmu = path_constants32(n, dim, pv)
    rat = unit_ratios(got, ref, sc, pv, betas)
    print(f"{label}: Cq {cq.max():.0f} Cmu {cmu.max():.0f}; worst err / (u32 S + abs): "
          + ", ".join(f"{k} {v:.3g}" for k, v in rat.items()))
    _, tol = X.check_exact(got, _folded(ref, sc, cq[:, None], cmu[:, None]), pv, betas, 1.0, 1.0,
                           f"    {label} against the counted bound (err / tol)")
    return rat, tol


def restate32(x, y, kinv, pm, pv, ls, betas, pts, min_var=1e-10, drop_half_row=None):
    """The kernel's specified numerics in numpy float32 (module docstring).  drop_half_row: a CPU mutant,
    W's diagonal not halved on that row."""
    x = np.asarray(x)
    pts = np.asarray(pts)
    y = np.asarray(y, dtype=np.float64)
    n, n_obj, m = x.shape[0], len(pm), pts.shape[0]
    z = x[0].astype(np.float64)
    xc = (x.astype(np.float64) - z).astype(F32)
    pc = (pts.astype(np.float64) - z).astype(F32)
    d = xc[None, :, :] - pc[:, None, :]
    d2 = (d * d).sum(-1, dtype=F32)
    out = {k: np.empty((n_obj, m)) for k in ("mu", "var", "std_mu", "std_var", "ucb")}
    acq = np.zeros(m)
    for o in range(n_obj):
        A = np.asarray(kinv, dtype=np.float64)[o, :n, :n]
        w = np.triu(0.5 * (A + A.T))
        w[np.diag_indices(n)] = 0.5 * np.diag(A)
        if drop_half_row is not None:
            w[drop_half_row, drop_half_row] = A[drop_half_row, drop_half_row]
        w = w.astype(F32)
        pv_o, pm_o = float(pv[o]), float(pm[o])
        nl2 = F32((-0.5 / (float(ls[o]) * float(ls[o]))) * 1.4426950408889634)
        lpv = F32(np.log2(pv_o))
        k = np.exp2(d2 * nl2 + lpv).astype(F32)
        alpha = (A @ (y[:n, o] - pm_o)).astype(F32)
        qh = np.einsum("mn,mn->m", k @ w.T, k, dtype=F32)
        mp = k @ alpha
        assert qh.dtype == F32 and mp.dtype == F32 and k.dtype == F32
        mu = pm_o + mp.astype(np.float64)
        var = np.maximum(pv_o - 2.0 * qh.astype(np.float64), min_var)
        smu = (mu - pm_o) * (1.0 / np.sqrt(pv_o))
        svar = var * (1.0 / pv_o)
        u = smu + float(betas[o]) * np.sqrt(np.abs(svar))
        acq = u if o == 0 else acq + u
        for name, v in (("mu", mu), ("var", var), ("std_mu", smu), ("std_var", svar), ("ucb", u)):
            out[name][o] = v
    out["acq"] = acq
    return out


# ---- the cases.  A case: the problem (x, y, Kinv, pm, pv, ls, betas), min_var, the candidate set's
# description `cand` (("grid", bounds) | ("f64" | "i64", points) | ("sobol", dim, n, scale)), the scored
# global indices idx and their points pts, the class, and -- computed once, on demand -- ref, sc, restated.

GRID_A = ((13, 11), (-5, 100))            # 143 candidates: two full 64-candidate tiles and a tail of 15
GRID_B = ((40, 30), (0, 0))
GRID_C = ((64, 48), (0, 0))
PEEL_N = (1, 16, 17, 48, 49, 64, 65)
EDGE_N = (1024, 1025, 1088)
_CASES = {}


def _grid_all(shape, lo):
    ii, jj = np.meshgrid(np.arange(shape[0]) + lo[0], np.arange(shape[1]) + lo[1], indexing="ij")
    return np.stack([ii.ravel(), jj.ravel()], axis=1).astype(np.int64)


def _kinv(x, pv, ls, jitter=O.KERNEL_JITTER):
    n, n_obj = x.shape[0], len(pv)
    km = np.zeros((n_obj, n, n))
    O.update_k(km, np.asarray(x, dtype=np.float64), 0, n, pv, ls)
    return np.stack([np.linalg.inv(km[o] + jitter * np.eye(n)) for o in range(n_obj)])


def _problem(rng, x, n_obj, ls, y_scale=30.0):
    """Random objectives (each at its own scale, so that pv differs) on the training rows x."""
    n = x.shape[0]
    scale = y_scale * (1.0 + 0.35 * np.arange(n_obj))
    y = rng.normal(size=(n, n_obj)) * scale + 5.0
    pm, pv = y.mean(0), y.var(0)
    if n == 1:                                      # one point has no spread: any positive prior
        pm, pv = y[0] - 1.0, np.full(n_obj, 4.0)
    ls = np.broadcast_to(np.asarray(ls, dtype=np.float64), (n_obj,)).copy()
    betas = rng.uniform(0.5, 2.5, size=n_obj)
    return dict(x=np.asarray(x, dtype=np.float64), y=y, pm=pm, pv=pv, ls=ls, betas=betas,
                Kinv=_kinv(x, pv, ls), min_var=1e-10)


def _grid_case(shape, lo, n, n_obj, ls, seed, idx=None):
    rng = np.random.default_rng(seed)
    allp = _grid_all(shape, lo)
    train = rng.choice(allp.shape[0], n, replace=False)
    d = _problem(rng, allp[train], n_obj, ls)
    d["cand"] = ("grid", [(lo[0], lo[0] + shape[0]), (lo[1], lo[1] + shape[1])])
    d["train_idx"] = train
    d["idx"] = np.arange(allp.shape[0]) if idx is None else idx(train, allp.shape[0], rng)
    d["pts"] = allp[d["idx"]]
    return d


def _edge_sample(train, total, rng, per_chunk=6, size=130):
    """Training points of the first, the 16th, the 17th and the last chunk, and every non-training point
    the sample allows."""
    n = train.size
    chunks = sorted({0, 15, (n - 1) // 64 if n > 1024 else 15, (n - 1) // 64})
    half = per_chunk // 2
    tr = np.concatenate([np.r_[train[64 * c:min(64 * c + 64, n)][:half], train[64 * c:min(64 * c + 64, n)][-half:]]
                         for c in chunks])
    free = np.setdiff1d(np.arange(total), train)
    free = free if free.size <= size - tr.size else np.sort(rng.choice(free, size - tr.size, replace=False))
    return np.unique(np.concatenate([tr, free]))


def _explicit_case(kind, dim, n, m, ls, seed, n_obj=2):
    """An explicit or Sobol set of m candidates of which n (a random subset) are the training rows."""
    rng = np.random.default_rng(seed)
    if kind == "sobol":
        from scipy.stats import qmc
        scale = 300.0
        allp = qmc.Sobol(dim, scramble=False).random(m) * scale       # lo = 0: lo + u scale, exactly
        cand = ("sobol", dim, m, scale)
    elif kind == "i64":
        allp = np.unique(rng.integers(0, 12, size=(2 * m, dim)), axis=0)
        allp = allp[rng.permutation(allp.shape[0])[:m]].astype(np.int64)
        cand = ("i64", allp)
    else:
        if dim == 1:        # a jittered lattice: no two points closer than 0.4
            allp = (np.arange(m) * 1.0 + rng.uniform(-0.3, 0.3, size=m))[rng.permutation(m), None] + 17.25
        else:
            allp = rng.uniform(0.0, 10.0, size=(m, dim)) + 3.0
        cand = ("f64", allp)
    assert allp.shape == (m, dim)
    train = rng.choice(m, n, replace=False)
    d = _problem(rng, allp[train], n_obj, ls)
    d.update(cand=cand, train_idx=train, idx=np.arange(m), pts=allp)
    return d


DIM_CASES = {          # name: (kind, dim, N, M, ls)
    "dim1-f64": ("f64", 1, 70, 200, (0.8, 0.6)),
    "dim3-f64": ("f64", 3, 97, 200, (1.5, 1.0)),
    "dim5-sobol": ("sobol", 5, 81, 256, (40.0, 30.0)),
    "dim7-i64": ("i64", 7, 130, 200, (3.0, 2.0)),
    "dim8-f64": ("f64", 8, 100, 200, (3.0, 2.5)),
}
RING_LS = (0.7, 0.8, 0.9, 1.0, 1.1, 1.2, 1.3, 1.4)


def _build(name):
    if name.startswith("peel-n"):
        return _grid_case(*GRID_A, int(name[6:]), 2, (1.5, 1.0), 100 + int(name[6:]))
    if name.startswith("edge-n"):
        return _grid_case(*GRID_B, int(name[6:]), 2, (0.7, 0.9), 200 + int(name[6:]), idx=_edge_sample)
    if name == "groups3-n2049":
        return _grid_case(*GRID_C, 2049, 1, (0.8,), 2049,
                          idx=lambda tr, tot, rng: np.unique(np.concatenate(
                              [tr[[0, 1, 63, 64, 1023, 1024, 2047, 2048]],
                               rng.choice(np.setdiff1d(np.arange(tot), tr), 62, replace=False)])))
    if name in DIM_CASES:
        kind, dim, n, m, ls = DIM_CASES[name]
        return _explicit_case(kind, dim, n, m, ls, sum(map(ord, name)))
    if name == "ring-nobj8":
        return _grid_case(*GRID_A, 81, 8, RING_LS, 81)
    if name == "ring-nobj1":
        d = case("ring-nobj8")
        return dict({k: d[k] for k in ("x", "cand", "train_idx", "idx", "pts", "min_var")},
                    y=d["y"][:, :1].copy(), pm=d["pm"][:1], pv=d["pv"][:1], ls=d["ls"][:1], betas=d["betas"][:1],
                    Kinv=d["Kinv"][:1].copy())
    if name == "skew-n65":
        # a non-symmetric K^-1: A plus a skew perturbation of 1e-3 |A|; A is data, nothing else changes
        d = {k: v for k, v in case("peel-n65").items() if k not in ("ref", "sc", "restated", "integer")}
        rng = np.random.default_rng(65)
        s = np.triu(rng.choice([-1.0, 1.0], size=d["Kinv"].shape), 1)
        return dict(d, Kinv=d["Kinv"] + 1e-3 * np.abs(d["Kinv"]) * (s - s.transpose(0, 2, 1)))
    if name == "floor32-n49":
        # float_type=np.float32: MIN_VARIANCE 1e-6; pv ~ 1 and a jitter of 1e-7, so that the posterior
        # variance at a training point (~ the jitter) is under the floor and away from the data is not
        rng = np.random.default_rng(49)
        allp = _grid_all(*GRID_A)
        train = rng.choice(allp.shape[0], 49, replace=False)
        d = _problem(rng, allp[train], 2, (1.2, 0.9), y_scale=1.0)
        d["Kinv"] = _kinv(d["x"], d["pv"], d["ls"], jitter=1e-7)
        d.update(cand=("grid", [(-5, 8), (100, 111)]), train_idx=train, idx=np.arange(143), pts=allp, min_var=1e-6)
        return d
    raise KeyError(name)


CASE_NAMES = tuple(f"peel-n{n}" for n in PEEL_N) + tuple(f"edge-n{n}" for n in EDGE_N) + ("groups3-n2049",) + \
    tuple(DIM_CASES) + ("ring-nobj1", "ring-nobj8", "skew-n65", "floor32-n49")


def case(name):
    """The case with its reference (exact_predict), scales and restatement, each computed once."""
    if name not in _CASES:
        d = _build(name)
        args = (d["x"], d["y"], d["Kinv"], d["pm"], d["pv"], d["ls"])
        d["pts"] = d["pts"][::X.SUBSAMPLE] if not X.LD_OK else d["pts"]
        d["idx"] = d["idx"][::X.SUBSAMPLE] if not X.LD_OK else d["idx"]
        d["ref"] = X.exact_predict(*args, d["betas"], d["pts"], min_var=d["min_var"])
        d["sc"] = scales32(*args, d["pts"])
        d["integer"] = d["sc"]["integer"]
        d["restated"] = restate32(*args, d["betas"], d["pts"], min_var=d["min_var"])
        _CASES[name] = d
    return _CASES[name]


def restated_ratios(name):
    d = case(name)
    return unit_ratios(d["restated"], d["ref"], d["sc"], d["pv"], d["betas"])


_R = {}


def tight_R(integer, output):
    """R of the tight rule for the class and the output ("var" or "mu"): the restatement's largest ratio of
    that output over the class's cases."""
    if not _R:
        for nm in CASE_NAMES:
            rat = restated_ratios(nm)
            for k in ("var", "mu"):
                key = (case(nm)["integer"], k)
                _R[key] = max(_R.get(key, 0.0), rat[k])
    return _R[(bool(integer), output)]


def f64_ratio_ceiling(n, dim):
    """What an f64 evaluation of the same case could reach at most in the unit ratios err / (u32 S + abs):
    exact_ref's chunk-major constant in units of u64 / u32 = 2^-29.  A device ratio a thousand times above it
    cannot come from an f64 kernel: the f32 kernel ran."""
    return max(X.path_constants("chunk-major", n, 0, dim)) * U64 / U32

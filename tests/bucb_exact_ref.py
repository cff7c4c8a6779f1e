"""Extended-precision reference of the hallucinated-observation update (bo_bucb_impl.h: the numeric core
of bo_select_batch_bucb, bo_select_batch_kb and bo_select_batch_gibbon), STAGE BY STAGE, and a counted
rounding-error bound per stage.  Helper module: no tests in it (tests/test_bucb_exact_ref.py pins it
on the CPU, tests/test_gpu_bucb_exact.py holds the device to it).

The reference.  Every stage takes the device's own outputs of the stage before it as DATA, read from
the workspace (tests/bucb_layout_model.py), together with kinv (the f64 array handed to the device, as
in tests/exact_ref.py).  Conditioning then enters only through the magnitudes of the terms, and every
bound holds at any cond(K).  Everything is evaluated in numpy.longdouble (64-bit significand; mpmath at
128 bits, on every SUBSAMPLE-th candidate, where the platform's long double is no wider than f64) and
compared with the device's f64 value without rounding the reference.

Throughout u = 2^-53, a = |diff|^2 / (2 l^2), k = pv exp(-a) the stage's own kernel value, and the
coordinates are the centred f64 values the device sees: xc = fl(x - x[0]), cc = fl(c - x[0]), one IEEE
subtraction each, which numpy reproduces bit for bit (bucb_prep_kernel, bo_cand_load<DIMP, true>).

  S0  bitwise: xc, pc[t] = cc[p_t], pick[t] = top_idx[t] - cand_offset (or -1), the call's mask = the
      caller's bits plus the picks.  (Asserted by the GPU tests themselves; centre() gives the values.)
  S1  bucb_pick_kernel: kx[o][f] = k_o(xc_f, pc_t), kp[o][r] = k_o(pc_r, pc_t), r <= t.
          tol = (C_e + C_a a) u k + 2^-1022
  S2  bucb_matvec_kernel: w_t = A kx, A = kinv and the device's kx as data.
          tol_i = C_w u sum_f |A_if| |kx_f|
  S3/S4  bucb_coef_kernel, thread 0.  Data: the device's kx, kp, w_0..w_t, rows A_s and d_s, s < t.
          e_r = kp_r - kx . w_r,   c_s = A_s . e,   g_s = c_s / d_s,   a = (unit row t) - sum_s g_s A_s,
          c_tt = e_t - sum_s c_s g_s,   d_t = max(c_tt, 0) + jitter
          tol_e    = C_e' u (|kp_r| + sum_f |kx_f w_rf|)
          tol_cs   = |A_s| . tol_e + (s + 1) u |A_s| . |e|
          tol_g    = tol_cs / d_s + u |g|
          tol_a[r] = sum_s (tol_g + 2u |g_s|) |A_s[r]| + u |a_r|
          tol_d    = tol_e[t] + sum_s (tol_cs |g| + |c_s| tol_g + 2u |c_s g|) + u d_t
      d_s is data, so nothing is linearised in a quantity that can vanish.  A step that the device
      leaves out (ok == 0: no pick, or d_t not positive and finite) must have a zero row, d_t = 1 and
      zero weights, exactly; it MAY be left out only when the reference's d_t is not above tol_d.
  S5  the weights: u_f = -sc sum_r a_r w_r[f], u_{N + r} = sc a_r, sc = 1 / sqrt(d_t), with the device's
      row t and d_t as data.
          tol_f = C_u u sc sum_r |a_r w_rf|          tail: 4u sc |a_r|
  S6  bucb_cand_kernel / gibbon_cand_kernel, every candidate: acc = sum over the N + t + 1 rows of
      k(row, c) u_row with the device's u as data, var^t = max(var^(t-1) - acc^2, min_var), var^(t-1)
      the device's var_out of the run with one pick fewer (the input `var` for t = 0).
          tol_acc = u sum_rows (C_r + C_a a) k |u_row|
          tol_var = 2 |acc| tol_acc + tol_acc^2 + 2u (|var^(t-1)| + acc^2)
  S7  bo_select_batch_bucb only: acq = sum_o std_mu_o + beta_o sqrt(|var_o| / pv_o) of the device's own
      var of the run with one pick fewer, for acq_out and top_val.
          tol = (n_obj + 4) u sum_o (|std_mu_o| + |beta_o| sqrt(|var_o| / pv_o))
      -- per term 1 / pv and the product (2u under the root: u), the root 1, the product with beta 1,
      the addition to std_mu 1: 4; then n_obj roundings of the running sum over the objectives.

kx, kp and u are overwritten at every pick: the state after pick t is read from a run of q' = t + 1
picks with var_out set (the device is deterministic: the picks of run q' are a prefix of run q's).

The constants are COUNTED from bayesopt_smart_amd/csrc/bo_bucb_impl.h: the longest chain of roundings
through which one term reaches the output.  L = ceil(N / 64).
  C_a, the exponent's argument (a-weighted: a relative error d in a is a relative error a d in k):
    nl2 = -0.5 / (ls ls) 1.4426950408889634 (fill_args): the square, the quotient, the product and
      the constant's own rounding                                                                    4
    the FMA sq nl2 + lpv rounds t = log2 k once, u |t| absolute: its share a log2 e, times ln 2       1
    the squared distance: the differences (u each, so 2u on every square, 2u on the sum)              2
      and one FMA per coordinate, each rounding a partial sum <= sq (a padded coordinate adds an
      exact zero)                                                                                 dim
    C_a = dim + 7.
  C_e, a pick vector's entry (bucb_pick_kernel):
    exp2 of the device library, 1 ulp                                                                 2
    lpv = log2 pv (fill_args; the host's log2 within 1 ulp, 2u |lpv|) and lpv's share of the FMA's
      rounding (u |lpv|): 3 ln 2 |log2 pv| u <= 2.08 u for 1/2 <= pv <= 2, which constants() asserts  3
    C_e = 5.
  C_w, the mat-vec (bucb_matvec_kernel): a lane's L FMAs, then the 6 additions of wave_sum; the last
    one is the stored value.  C_w = L + 6.
  C_e' (bucb_coef_kernel): the same dot product, L + 6, and the subtraction from kp_r.  C_e' = L + 7.
  C_u: sc = 1 / sqrt(d_t): the device library's root within 1 ulp 2, the quotient 1; the t + 1 FMAs
    over r; the product -sc s 1.  C_u = t + 5.  The tail sc a_r has the root, the quotient and the
    product: the stated 4u.
  C_r, one term k u_row of the candidate pass: the N + t + 1 FMAs of the row loop (one thread, row
    order: staging in chunks does not change the chain), and the kernel value by exp2_tab with
    lpv = log2 pv, which tests/exact_ref.py counts as 11.  C_r = N + t + 12.
None may exceed 2 (N + q) + 2 dim + 64 (q = t + 1 here); constants() asserts it.  The bounds are first
order in u; the tests print every stage's worst err / tol.
"""
import contextlib

import numpy as np

U = 2.0 ** -53
TINY = 2.0 ** -1022
LD = np.longdouble
LD_OK = bool(np.finfo(LD).eps <= 2.0 ** -63)
# where long double is no wider than f64 the reference is mpmath at 128 bits, and the candidate pass is
# scored on every SUBSAMPLE-th candidate
SUBSAMPLE = 1 if LD_OK else 16
MP_BITS = 128
STAGES = ("S1", "S2", "S4", "S5", "S6")

CHUNK_DOUBLES = 4096        # kChunkDoubles


def nob_of(n_obj):
    """The candidate kernels' NOB: objectives padded to 1, 2, 3, 4 or 8."""
    return n_obj if n_obj <= 4 else 8


def chunk_rows(dim, n_obj):
    """RC of bucb_cand_kernel / gibbon_cand_kernel: rows of [X; picks] per staged chunk."""
    return (CHUNK_DOUBLES // (((dim + 1) & ~1) + nob_of(n_obj))) & ~3


def constants(n, t, dim, pv):
    """The module docstring's counts for step t of a call over n training rows."""
    pv = np.asarray(pv, dtype=np.float64)
    assert np.all((pv >= 0.5) & (pv <= 2.0)), "C_e's count of lpv = log2 pv holds for 1/2 <= pv <= 2"
    lanes = -(-n // 64)
    c = {"C_e": 5, "C_a": dim + 7, "C_w": lanes + 6, "C_e'": lanes + 7, "C_u": t + 5, "C_r": n + t + 12}
    cap = 2 * (n + t + 1) + 2 * dim + 64
    assert all(v <= cap for v in c.values()), (c, cap)
    return {k: float(v) for k, v in c.items()}


# ------------------------------------------------------------------------------ extended arithmetic
class _LongDouble:
    name = "longdouble"
    eps = float(np.finfo(LD).eps)

    @staticmethod
    def prec():
        return contextlib.nullcontext()

    @staticmethod
    def arr(a):
        return np.asarray(a, dtype=np.float64).astype(LD)      # every f64 exactly

    s = staticmethod(lambda v: LD(float(v)))
    exp = staticmethod(np.exp)
    sqrt = staticmethod(np.sqrt)

    @staticmethod
    def f64(a):
        return np.asarray(a, dtype=LD).astype(np.float64)

    @staticmethod
    def zeros(shape):
        return np.zeros(shape, dtype=LD)


class _Mpmath:
    name = "mpmath"
    eps = 2.0 ** -(MP_BITS - 1)

    @staticmethod
    def prec():
        import mpmath as mp
        return mp.workprec(MP_BITS)

    @staticmethod
    def arr(a):
        import mpmath as mp
        a = np.asarray(a, dtype=np.float64)
        out = np.empty(a.shape, dtype=object)
        out.ravel()[:] = [mp.mpf(float(v)) for v in a.ravel()]
        return out if a.ndim else out[()]

    @staticmethod
    def s(v):
        import mpmath as mp
        return mp.mpf(float(v))

    @staticmethod
    def exp(a):
        import mpmath as mp
        return np.frompyfunc(mp.exp, 1, 1)(a)

    @staticmethod
    def sqrt(a):
        import mpmath as mp
        return np.frompyfunc(mp.sqrt, 1, 1)(a)

    @staticmethod
    def f64(a):
        a = np.asarray(a, dtype=object)
        out = np.empty(a.shape, dtype=np.float64)
        out.ravel()[:] = [float(v) for v in a.ravel()]
        return out

    @staticmethod
    def zeros(shape):
        import mpmath as mp
        out = np.empty(shape, dtype=object)
        out.ravel()[:] = [mp.mpf(0) for _ in range(out.size)]
        return out


EXT = _LongDouble if LD_OK else _Mpmath


def _dot(a, b):
    """a @ b for the extended types (object arrays have no BLAS; this is the plain sum of products)."""
    return a @ b


def kern(E, rows, c, pv_o, ls_o):
    """k [M, R] (extended) and a [M, R] (f64) between the centred points c [M, dimp] and rows [R, dimp]."""
    d = E.arr(rows)[None, :, :] - E.arr(c)[:, None, :]
    sq = (d * d).sum(axis=-1)
    a = sq / (2 * E.s(ls_o) * E.s(ls_o))
    return E.exp(-a) * E.s(pv_o), E.f64(a)


def centre(x, pts):
    """(xc [N, dimp], cc [M, dimp]) in f64: the device's centred coordinates, padded coordinate 0.
    pts: the candidates' values as the device decodes them (integers exactly for grid / i64)."""
    x = np.asarray(x, dtype=np.float64)
    dim = x.shape[1]
    dimp = (dim + 1) & ~1
    xc = np.zeros((x.shape[0], dimp))
    cc = np.zeros((pts.shape[0], dimp))
    xc[:, :dim] = x - x[0]
    cc[:, :dim] = np.asarray(pts).astype(np.float64) - x[0]
    return xc, cc


def _ratio(err, tol):
    """max err / tol; 0 where err == 0 (tol may be 0 there); inf for a NaN."""
    err = np.atleast_1d(np.asarray(err, dtype=np.float64))
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), err.shape)
    with np.errstate(all="ignore"):
        r = np.where(err == 0.0, 0.0, err / tol)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


def _exact(ok):
    return 0.0 if ok else np.inf


# ---------------------------------------------------------------------------------------- the stages
# pb: the problem -- x [N, dim], pts [M, dim], pv, ls, beta [n_obj], jitter, min_var, kinv [n_obj, N, N]
#     (the N x N blocks), std_mu, var [n_obj, M] (the call's inputs).
# st: the state after pick t -- t, xc, pc, kx, kp, wv, coef, dd, u, ok, pick (the workspace regions of a
#     run of t + 1 picks, bucb_layout_model's shapes) and var (that run's var_out [n_obj, M]).

def _consts(pb, st):
    return constants(pb["x"].shape[0], st["t"], pb["x"].shape[1], pb["pv"])


def stage1(pb, st, E=None):
    E = E or EXT
    t, c = st["t"], _consts(pb, st)
    worst = 0.0
    with E.prec():
        for o in range(len(pb["pv"])):
            got = [(st["kx"][o], st["xc"]), (st["kp"][o, :t + 1], st["pc"][:t + 1])]
            if st["pick"][t] < 0:                              # no candidate left: zeros
                worst = max(worst, _exact(all(np.all(g == 0.0) for g, _ in got)))
                continue
            for g, rows in got:
                k, a = kern(E, rows, st["pc"][t:t + 1], pb["pv"][o], pb["ls"][o])
                tol = (c["C_e"] + c["C_a"] * a[0]) * U * E.f64(k[0]) + TINY
                worst = max(worst, _ratio(E.f64(abs(E.arr(g) - k[0])), tol))
    return worst


def stage2(pb, st, E=None):
    E = E or EXT
    t, c = st["t"], _consts(pb, st)
    worst = 0.0
    with E.prec():
        for o in range(len(pb["pv"])):
            w = _dot(E.arr(pb["kinv"][o]), E.arr(st["kx"][o]))
            tol = c["C_w"] * U * (np.abs(pb["kinv"][o]) @ np.abs(st["kx"][o]))
            worst = max(worst, _ratio(E.f64(abs(E.arr(st["wv"][o, t]) - w)), tol))
    return worst


def coef_reference(E, kx, kp, w, rows, d, jitter, c_e1):
    """Row t of A, c_tt and d_t (extended) with tol_a, tol_d (f64), from kx [N], kp [t + 1], w [t + 1, N],
    the earlier rows [t][>= t] (row s read up to s) and d [t], all f64 data."""
    t = kp.shape[0] - 1
    e = E.arr(kp) - _dot(E.arr(w), E.arr(kx))
    tol_e = c_e1 * U * (np.abs(kp) + np.abs(w) @ np.abs(kx))
    e64 = np.abs(E.f64(e))
    a = E.zeros(t + 1)
    a[t] = a[t] + 1
    tol_a = np.zeros(t + 1)
    ctt, tol_d = e[t], tol_e[t]
    for s in range(t):
        row = E.arr(rows[s, :s + 1])
        ab = np.abs(rows[s, :s + 1])
        cs = _dot(row, e[:s + 1])
        tol_cs = ab @ tol_e[:s + 1] + (s + 1) * U * (ab @ e64[:s + 1])
        g = cs / E.s(d[s])
        g64, cs64 = abs(float(g)), abs(float(cs))
        tol_g = tol_cs / d[s] + U * g64
        a[:s + 1] = a[:s + 1] - row * g
        tol_a[:s + 1] += (tol_g + 2 * U * g64) * ab
        ctt = ctt - cs * g
        tol_d += tol_cs * g64 + cs64 * tol_g + 2 * U * cs64 * g64
    tol_a += U * np.abs(E.f64(a))
    dt = (ctt if ctt > 0 else ctt * 0) + E.s(jitter)
    tol_d += U * abs(float(dt))
    return a, ctt, dt, tol_a, tol_d


def stage4(pb, st, E=None):
    """S3/S4: row t of coef and dd[t].  Also returns whether the reference lets the step be left out."""
    E = E or EXT
    t, c = st["t"], _consts(pb, st)
    worst = 0.0
    with E.prec():
        for o in range(len(pb["pv"])):
            a, _, dt, tol_a, tol_d = coef_reference(E, st["kx"][o], st["kp"][o, :t + 1], st["wv"][o, :t + 1],
                                                    st["coef"][o, :t, :t + 1], st["dd"][o, :t], pb["jitter"],
                                                    c["C_e'"])
            row, d_dev = st["coef"][o, t, :t + 1], st["dd"][o, t]
            if not st["ok"][o]:                                # left out: exact, and only where allowed
                allowed = st["pick"][t] < 0 or not (float(dt) - tol_d > 0)
                worst = max(worst, _exact(allowed and np.all(row == 0.0) and d_dev == 1.0))
                continue
            worst = max(worst, _exact(st["pick"][t] >= 0),
                        _ratio(E.f64(abs(E.arr(row) - a)), tol_a), _ratio(E.f64(abs(E.s(d_dev) - dt)), tol_d))
    return worst


def stage5(pb, st, E=None):
    E = E or EXT
    t, c, n = st["t"], _consts(pb, st), pb["x"].shape[0]
    worst = 0.0
    with E.prec():
        for o in range(len(pb["pv"])):
            u_dev = st["u"][o, :n + t + 1]
            if not st["ok"][o]:
                worst = max(worst, _exact(np.all(u_dev == 0.0)))
                continue
            row, w = st["coef"][o, t, :t + 1], st["wv"][o, :t + 1]
            sc = 1 / E.sqrt(E.s(st["dd"][o, t]))
            sc64 = float(sc)
            ref = _dot(E.arr(row), E.arr(w)) * (-sc)
            tol = c["C_u"] * U * sc64 * (np.abs(row) @ np.abs(w))
            worst = max(worst, _ratio(E.f64(abs(E.arr(u_dev[:n]) - ref)), tol),
                        _ratio(E.f64(abs(E.arr(u_dev[n:]) - E.arr(row) * sc)), 4 * U * sc64 * np.abs(row)))
    return worst


def selection(m):
    """The candidates the candidate pass is scored on."""
    return np.arange(0, m, SUBSAMPLE)


def stage6(pb, st, var_prev, E=None, sel=None):
    """var of the run (st["var"]) against max(var_prev - acc^2, min_var) over the candidates `sel`."""
    E = E or EXT
    t, c, n = st["t"], _consts(pb, st), pb["x"].shape[0]
    sel = selection(pb["pts"].shape[0]) if sel is None else sel
    _, cc = centre(pb["x"], pb["pts"])
    cache = pb.setdefault("_kern", {})
    worst = 0.0
    with E.prec():
        for o in range(len(pb["pv"])):
            got, prev = st["var"][o, sel], var_prev[o, sel]
            if not st["ok"][o]:
                worst = max(worst, _exact(got.tobytes() == prev.tobytes()))
                continue
            key = (E.name, o, sel.tobytes())
            if key not in cache:                               # the training rows' values serve every t
                cache[key] = kern(E, st["xc"], cc[sel], pb["pv"][o], pb["ls"][o])
            kp_, ap_ = kern(E, st["pc"][:t + 1], cc[sel], pb["pv"][o], pb["ls"][o])
            k = np.concatenate([cache[key][0], kp_], axis=1)
            a = np.concatenate([cache[key][1], ap_], axis=1)
            uo = st["u"][o, :n + t + 1]
            acc = _dot(k, E.arr(uo))
            tol_acc = U * (((c["C_r"] + c["C_a"] * a) * E.f64(k)) @ np.abs(uo))
            pe = E.arr(prev)
            var = pe - acc * acc
            floor = E.s(pb["min_var"])
            var = np.where(var > floor, var, floor)
            acc64 = np.abs(E.f64(acc))
            tol = 2 * acc64 * tol_acc + tol_acc ** 2 + 2 * U * (np.abs(prev) + acc64 ** 2)
            worst = max(worst, _ratio(E.f64(abs(E.arr(got) - var)), tol))
    return worst


def stage7(pb, var_prev, got, idx=None, E=None):
    """S7: `got` [len(idx)] against the summed UCB of (std_mu, var_prev) at the candidates idx."""
    E = E or EXT
    idx = np.arange(pb["pts"].shape[0]) if idx is None else np.asarray(idx)
    n_obj = len(pb["pv"])
    with E.prec():
        acq, mag = 0, 0.0
        for o in range(n_obj):
            root = E.sqrt(abs(E.arr(var_prev[o, idx])) / E.s(pb["pv"][o]))
            acq = acq + E.arr(pb["std_mu"][o, idx]) + root * E.s(pb["beta"][o])
            mag = mag + np.abs(pb["std_mu"][o, idx]) + abs(pb["beta"][o]) * E.f64(root)
        return _ratio(E.f64(abs(E.arr(got) - acq)), (n_obj + 4) * U * mag)


def check_step(pb, st, var_prev, E=None, sel=None):
    """dict stage -> worst err / tol of one step."""
    return {"S1": stage1(pb, st, E), "S2": stage2(pb, st, E), "S4": stage4(pb, st, E), "S5": stage5(pb, st, E),
            "S6": stage6(pb, st, var_prev, E, sel)}


def merge(worst, step):
    for k, v in step.items():
        worst[k] = max(worst.get(k, 0.0), v)
    return worst


def report(label, worst):
    print(f"{label}: worst err / tol " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


# ------------------------------------------------------------- the recursion from scratch, extended
def chol_inverse(E, k):
    """inv(k) of a symmetric positive definite extended matrix by Cholesky."""
    n = k.shape[0]
    low = E.zeros((n, n))
    for j in range(n):
        low[j, j] = E.sqrt(k[j, j] - (low[j, :j] * low[j, :j]).sum())
        for i in range(j + 1, n):
            low[i, j] = (k[i, j] - (low[i, :j] * low[j, :j]).sum()) / low[j, j]
    y = E.zeros((n, n))                                        # low y = I
    for j in range(n):
        for i in range(j, n):
            rhs = (1 if i == j else 0) - (low[i, j:i] * y[j:i, j]).sum()
            y[i, j] = rhs / low[i, i]
    return _dot(y.T, y)


def gram(E, pts_c, pv_o, ls_o, jitter):
    k, _ = kern(E, pts_c, pts_c, pv_o, ls_o)
    for i in range(k.shape[0]):
        k[i, i] = k[i, i] + E.s(jitter)
    return k


def compose(E, xc, cc, picks, pv_o, ls_o, jitter, var0):
    """S1..S6 chained in extended precision with A = the extended inverse of K + jitter I and no clamp:
    var [len(picks), M] after every pick, for one objective; var0 [M]: the unconditioned variance (extended)."""
    n = xc.shape[0]
    inv = chol_inverse(E, gram(E, xc, pv_o, ls_o, jitter))
    kall, _ = kern(E, xc, cc, pv_o, ls_o)                       # [M, N]
    var = var0
    out, ws, rows, ds = [], [], [], []
    for t, p in enumerate(picks):
        pc = cc[list(picks[:t + 1])]
        kx = kern(E, xc, cc[p:p + 1], pv_o, ls_o)[0][0]
        kp = kern(E, pc, cc[p:p + 1], pv_o, ls_o)[0][0]
        ws.append(_dot(inv, kx))
        e = kp - np.array([(kx * w).sum() for w in ws])
        a = E.zeros(t + 1)
        a[t] = a[t] + 1
        ctt = e[t]
        for s in range(t):
            cs = (rows[s] * e[:s + 1]).sum()
            g = cs / ds[s]
            a[:s + 1] = a[:s + 1] - rows[s] * g
            ctt = ctt - cs * g
        dt = ctt + E.s(jitter)
        rows.append(a)
        ds.append(dt)
        sc = 1 / E.sqrt(dt)
        u = np.concatenate([sum(ws[r] * a[r] for r in range(t + 1)) * (-sc), a * sc])
        kpick, _ = kern(E, pc, cc, pv_o, ls_o)
        acc = _dot(np.concatenate([kall, kpick], axis=1), u)
        var = var - acc * acc
        out.append(var)
    return out


def augmented(E, xc, cc, picks, pv_o, ls_o, jitter):
    """(var, S) [M]: pv - k^T inv(K_aug + jitter I) k over [X; picks] in extended precision, and the
    cancellation scale S = pv + sum |k_i| |inv_ij| |k_j|."""
    pts = np.concatenate([xc, cc[list(picks)]]) if len(picks) else xc
    inv = chol_inverse(E, gram(E, pts, pv_o, ls_o, jitter))
    k, _ = kern(E, pts, cc, pv_o, ls_o)
    var = -(_dot(k, inv) * k).sum(axis=1) + E.s(pv_o)
    return var, (_dot(abs(k), abs(inv)) * abs(k)).sum(axis=1) + E.s(pv_o)


# ------------------------------------------------------------ the device recursion emulated in f64
def _fma(a, b, c):
    """fl(a b + c) with one rounding where long double is wide (the product's 2^-64 is 2^-11 u);
    two roundings otherwise."""
    if LD_OK:
        return (np.asarray(a, dtype=np.float64).astype(LD) * np.asarray(b, dtype=np.float64).astype(LD)
                + np.asarray(c, dtype=np.float64).astype(LD)).astype(np.float64)
    return np.asarray(a) * np.asarray(b) + np.asarray(c)


def _wave_dot(a, b):
    """sum a_f b_f over the last axis in bucb_matvec_kernel's order: lane f % 64 adds its terms by FMA,
    then the xor tree."""
    n = a.shape[-1]
    pad = -(-n // 64) * 64 - n
    shape = np.broadcast_shapes(a.shape, b.shape)
    a = np.concatenate([np.broadcast_to(a, shape), np.zeros(shape[:-1] + (pad,))], axis=-1)
    b = np.concatenate([np.broadcast_to(b, shape), np.zeros(shape[:-1] + (pad,))], axis=-1)
    a = a.reshape(shape[:-1] + (-1, 64))
    b = b.reshape(shape[:-1] + (-1, 64))
    s = np.zeros(shape[:-1] + (64,))
    for c in range(a.shape[-2]):
        s = _fma(a[..., c, :], b[..., c, :], s)
    lane = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        s = s + s[..., lane ^ m]
    return s[..., 0]


def _sqdist(rows, c):
    """[M, R]: the squared distance by one FMA per padded coordinate."""
    sq = np.zeros((c.shape[0], rows.shape[0]))
    for k in range(rows.shape[1]):
        d = rows[None, :, k] - c[:, None, k]
        sq = _fma(d, d, sq)
    return sq


def emulate(pb, q, picks=None, mask=None, mut=None, mut_t=None):
    """The device recursion in numpy f64, in the device's order of operations (numpy's exp2 for both
    kernel-value forms).  Returns (states, vars): states[t] as the stages take them, vars[t] = var after
    pick t.  picks: take these instead of the arg-max of the summed UCB.  mut: one of the mutations of
    tests/test_bucb_exact_ref.py, applied at step mut_t (None: every step)."""
    x, pv, ls = pb["x"], np.asarray(pb["pv"]), np.asarray(pb["ls"])
    n, dim = x.shape
    n_obj, m = len(pv), pb["pts"].shape[0]
    xc, cc = centre(x, pb["pts"])
    nl2 = -0.5 / (ls * ls) * 1.4426950408889634
    lpv = np.log2(pv)
    rc = chunk_rows(dim, n_obj)
    taken = np.zeros(m, dtype=bool) if mask is None else np.asarray(mask, dtype=bool).copy()
    var = pb["var"].copy()
    pc = np.zeros((q, xc.shape[1]))
    wv = np.full((n_obj, q, n), np.nan)
    coef = np.full((n_obj, q, q), np.nan)
    dd = np.full((n_obj, q), np.nan)
    pick = np.full(q, -1, dtype=np.int64)
    states, out_vars = [], []
    for t in range(q):
        on = mut is not None and (mut_t is None or mut_t == t)
        if picks is not None:
            p = int(picks[t])
        else:
            acq = (pb["std_mu"] + np.asarray(pb["beta"])[:, None] * np.sqrt(np.abs(var * (1.0 / pv)[:, None]))).sum(0)
            free = np.flatnonzero(~taken)
            p = int(free[np.argmax(acq[free])]) if free.size else -1
        pick[t] = p
        if p >= 0:
            taken[p] = True
            pc[t] = cc[p]
        kx = np.zeros((n_obj, n))
        kp = np.full((n_obj, q), np.nan)
        kp[:, :t + 1] = 0.0
        if p >= 0:
            for o in range(n_obj):
                kx[o] = np.exp2(_fma(_sqdist(xc, pc[t:t + 1])[0], nl2[o], lpv[o]))
                kp[o, :t + 1] = np.exp2(_fma(_sqdist(pc[:t + 1], pc[t:t + 1])[0], nl2[o], lpv[o]))
        u = np.zeros((n_obj, n + q))
        ok = np.zeros(n_obj, dtype=np.int32)
        for o in range(n_obj):
            wv[o, t] = _wave_dot(pb["kinv"][o], kx[o][None, :])
            if on and mut == "w_entry":
                i = int(np.argmax(np.abs(wv[o, t])))
                wv[o, t, i] *= 1.0 + 1e-12
            e = kp[o, :t + 1] - _wave_dot(wv[o, :t + 1], kx[o][None, :])
            a = np.zeros(t + 1)
            a[t] = 1.0
            ctt = e[t]
            for s in range(t):
                cs = 0.0
                for r in range(s + 1):
                    cs = float(_fma(coef[o, s, r], e[r], cs))
                g = cs / dd[o, s]
                a[:s + 1] = _fma(-g, coef[o, s, :s + 1], a[:s + 1])
                ctt = float(_fma(-cs, g, ctt))
            dt = max(ctt, 0.0) + pb["jitter"]
            if on and mut == "no_jitter":
                dt = max(ctt, 0.0)
            if on and mut == "no_clamp":
                dt = ctt + pb["jitter"]
            fin = p >= 0 and ctt == ctt and 0.0 < dt < np.inf
            coef[o, t, :t + 1] = a if fin else 0.0
            dd[o, t] = dt if fin else 1.0
            ok[o] = 1 if fin else 0
            if fin:
                sc = 1.0 / np.sqrt(dt)
                s_ = np.zeros(n)
                for r in range(t + 1):
                    s_ = _fma(a[r], wv[o, r], s_)
                u[o, :n] = -sc * s_
                u[o, n:n + t + 1] = sc * a
                if on and mut == "u_entry":
                    i = int(np.argmax(np.abs(u[o, :n])))
                    u[o, i] *= 1.0 + 1e-12
        rows = np.concatenate([xc, pc[:t + 1]])
        sq = _sqdist(rows, cc)
        skip = {"drop_chunk_row": rc - 1, "drop_pick_row": n + t}.get(mut if on else None)
        for o in range(n_obj):
            if not ok[o]:
                continue
            k = np.exp2(_fma(sq, nl2[o], lpv[o]))
            acc = np.zeros(m)
            for f in range(rows.shape[0]):
                if f != skip:
                    acc = _fma(k[:, f], u[o, f], acc)
            var[o] = np.maximum(_fma(-acc, acc, var[o]), pb["min_var"])
        states.append(dict(t=t, xc=xc, pc=pc[:t + 1].copy(), kx=kx, kp=kp[:, :t + 1].copy(),
                           wv=wv[:, :t + 1].copy(), coef=coef[:, :t + 1, :t + 1].copy(), dd=dd[:, :t + 1].copy(),
                           u=u[:, :n + t + 1].copy(), ok=ok, pick=pick[:t + 1].copy(), var=var.copy()))
        out_vars.append(var.copy())
    return states, out_vars


# ------------------------------------------------------------ the problems the CPU and GPU tests share
def fitted(x, pv, ls, jitter, want_cond=True):
    """kinv [n_obj, N, N] = inv(K_o + jitter I) by LAPACK in f64, and the worst cond(K_o + jitter I) (0 unless want_cond)."""
    d = x[:, None, :] - x[None, :, :]
    sq = (d * d).sum(-1)
    kinv = np.empty((len(pv), x.shape[0], x.shape[0]))
    cond = 0.0
    for o in range(len(pv)):
        k = pv[o] * np.exp(-0.5 * sq / (ls[o] * ls[o]))
        kinv[o] = np.linalg.inv(k + jitter * np.eye(x.shape[0]))
        if want_cond:
            cond = max(cond, float(np.linalg.cond(k + jitter * np.eye(x.shape[0]))))
    return kinv, cond


def problem(x, pts, n_obj, ls, seed, jitter=1e-6, min_var=1e-10, kinv_jitter=None, kinv=None, want_cond=True):
    """The inputs of one call over the candidates' values pts [M, dim]: pv in [0.6, 1.7], beta 2, std_mu
    random (so that the picks scatter), var = max(pv - k^T kinv k, min_var) in f64 -- data, like kinv."""
    rng = np.random.default_rng(seed)
    x = np.ascontiguousarray(x, dtype=np.float64)
    pv = np.array([1.3, 0.7, 1.1, 0.9, 1.7, 0.6, 1.0, 1.45])[:n_obj]
    ls = np.broadcast_to(np.asarray(ls, dtype=np.float64), (n_obj,)).copy()
    cond = float("nan")
    if kinv is None:
        kinv, cond = fitted(x, pv, ls, jitter if kinv_jitter is None else kinv_jitter, want_cond)
    p64 = np.asarray(pts).astype(np.float64)
    d = p64[:, None, :] - x[None, :, :]
    sq = (d * d).sum(-1)
    var = np.empty((n_obj, p64.shape[0]))
    for o in range(n_obj):
        k = pv[o] * np.exp(-0.5 * sq / (ls[o] * ls[o]))
        var[o] = np.maximum(pv[o] - ((k @ kinv[o]) * k).sum(1), min_var)
    return dict(x=x, pts=np.asarray(pts), pv=pv, ls=ls, beta=np.full(n_obj, 2.0), jitter=jitter, min_var=min_var,
                kinv=np.ascontiguousarray(kinv), std_mu=rng.standard_normal((n_obj, p64.shape[0])), var=var,
                cond=cond)

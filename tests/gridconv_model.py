"""numpy mirror of the grid-convolution predict path (bayesopt_smart_amd/csrc/bo_gridconv.hip) and
the problems its tests share.

The mirror follows the kernels' own order and addressing: the training points bucketed by column
(stable), per tau the pair list in (n ascending, m in bucket order) order accumulated
sequentially over the parity-split E table, then the two contractions in ascending k-blocks of 16
over the parity-split column table / the H table.  (numpy has no fused multiply-add and sums a
k-block in its own order: the mirror shares the kernels' grouping, not their last bit.)
"""

import numpy as np

from oracle import oracle_np as O

MARGIN = 1.15           # bo_predict.hip: kConvMargin
MAX_N = 4096            # kConvMaxN
LDS_BYTES = 160 * 1024
PAIR_CHUNK = 256        # bo_gridconv.hip: conv_lds_admits, the plan's frozen admission bound (the LDS of
PAIR_WAVES = 8          # no kernel): 8 x 256 = 2048 doubles and as many ints beside the tables of R, C and n


def conv_planned(shape, n, n_obj, offset=0, count=None, mode="auto"):
    """The host plan's decision (bo_predict.hip plan_gridconv): is the grid-convolution path
    planned for this call?  (Whether it then runs is the device flag's: every training point a
    grid point.)"""
    if len(shape) != 2 or mode not in ("auto", "auto-conv"):
        return False
    R, C = shape
    count = R * C - offset if count is None else count
    if count <= 0 or R > 1 << 15 or C > 1 << 15 or n > MAX_N:
        return False
    if offset < 0 or offset + count > R * C:
        return False
    Cpad, LT, NP = -(-C // 64) * 64, -(-(2 * C - 1) // 16) * 16, -(-n // 16) * 16
    lds_setup = (C + 1 + n + 256) * 4
    lds_pair = (4 * R + PAIR_WAVES * PAIR_CHUNK) * 8 + (C + 1 + 3 * n + PAIR_WAVES * PAIR_CHUNK) * 4
    lds_contract = (2 * (Cpad + LT // 2) + Cpad + C) * 8 + NP * 4
    if max(lds_setup, lds_pair, lds_contract) > LDS_BYTES:
        return False
    if mode == "auto-conv":
        return True
    us_conv, us_old = gate_times(shape, n, n_obj, offset, count)
    return MARGIN * us_conv < us_old


def gate_times(shape, n, n_obj, offset=0, count=None):
    """The gate's modelled times in microseconds (new sequence, chunk-major kernel)."""
    R, C = shape
    count = R * C - offset if count is None else count
    nrows = (offset + count - 1) // C - offset // C + 1
    nch = -(-n // 32)
    flops = n_obj * 1024.0 * nch * (nch + 1)
    us_old = 25.0 + (((count + 63) // 64 + 255) // 256) * 64.0 * (flops / 273.0e3 + 0.038)
    ldr, Cpad = -(-nrows // 16) * 16, -(-C // 64) * 64
    LT, NP = -(-(2 * C - 1) // 16) * 16, -(-n // 16) * 16
    pair = 2.2 * (0.5 * n * (n + 1) / (2 * C - 1)) * ((ldr + 1023) // 1024) * ((n_obj * (2 * C - 1) + 4095) // 4096)
    contract = (((ldr // 16) * (Cpad // 64) + 1023) // 1024) * 2048.0 * (LT + NP) * n_obj / 48.8e3
    return 60.0 + pair + contract, us_old


def lattice_problem(shape, lo, n, n_obj, seed, ls=None, lattice=4, step=3):
    """Training points on the grid `shape` at `lo`: a lattice x lattice block (spacing `step`, so
    that many pairs share a midpoint) plus random distinct grid points, n in all; random
    objectives; K well conditioned (cond < 1e6, the parity rule's domain)."""
    rng = np.random.default_rng(seed)
    R, C = shape
    pts = {(2 + step * a, 1 + step * b) for a in range(lattice) for b in range(lattice)
           if 2 + step * a < R and 1 + step * b < C}
    pts = sorted(pts)[:n]
    have = set(pts)
    while len(pts) < n:
        p = (int(rng.integers(R)), int(rng.integers(C)))
        if p not in have:
            have.add(p)
            pts.append(p)
    rel = np.array(pts, dtype=np.int64)[rng.permutation(n)]
    x = (rel + np.asarray(lo, dtype=np.int64)).astype(np.float64)
    y = rng.normal(size=(n, n_obj)) * 30 + 5
    pm, pv = y.mean(0), y.var(0)
    if n == 1:                                       # one point has no spread: any positive prior
        pm, pv = y[0] - 1.0, np.full(n_obj, 4.0)
    ls = rng.uniform(1.2, 2.2, size=n_obj) if ls is None else np.asarray(ls, dtype=np.float64)
    betas = rng.uniform(0.5, 2.5, size=n_obj)
    km = np.zeros((n_obj, n, n))
    O.update_k(km, x, 0, n, pv, ls)
    assert max(np.linalg.cond(km[o] + 1e-6 * np.eye(n)) for o in range(n_obj)) < 1e6
    kinv = O.invert_k(n, km)
    return dict(x=x, y=y, pm=pm, pv=pv, ls=ls, betas=betas, Kinv=kinv, rel=rel)


def grid_points(shape, lo):
    ii, jj = np.meshgrid(np.arange(shape[0]) + lo[0], np.arange(shape[1]) + lo[1], indexing="ij")
    return np.stack([ii.ravel(), jj.ravel()], axis=1).astype(np.int64)


def model_predict(x, y, kinv, pm, pv, ls, betas, shape, lo, min_var=1e-10):
    """mu, var, acq over the whole grid [R][C] by the grid-convolution path's arithmetic."""
    R, C = shape
    n, n_obj = x.shape[0], len(pm)
    r = (x[:, 0] - lo[0]).astype(np.int64)
    c = (x[:, 1] - lo[1]).astype(np.int64)
    assert ((r >= 0) & (r < R) & (c >= 0) & (c < C)).all()
    order = np.argsort(c, kind="stable")                       # conv_setup_block
    cstart = np.searchsorted(c[order], np.arange(C + 1))
    LT, NP, Cpad = -(-(2 * C - 1) // 16) * 16, -(-n // 16) * 16, -(-C // 64) * 64
    HB, R2 = Cpad + LT // 2, 2 * R
    rows = np.arange(R)
    mu = np.empty((n_obj, R * C))
    var = np.empty((n_obj, R * C))
    acq = np.zeros(R * C)
    for o in range(n_obj):
        nhl = -0.5 / ls[o] ** 2
        # pair stage: tabE[par * 2R + h] = E(2h + par - (2R - 2))
        t = np.arange(2 * R2)
        par, h = t // R2, t % R2
        tabE = np.exp(0.5 * nhl * (2 * h + par - (R2 - 2)).astype(np.float64) ** 2)
        T = np.zeros((LT, R))
        for tau in range(2 * C - 1):
            hi, low = np.zeros(R), np.zeros(R)                # compensated (two-sum) row sums
            for a in range(n):
                pc = tau - c[a]
                if pc < 0 or pc >= C:
                    continue
                for m in order[cstart[pc]:cstart[pc + 1]]:
                    if m < a:
                        continue
                    sym = kinv[o, a, a] if m == a else kinv[o, a, m] + kinv[o, m, a]
                    d2 = float((r[a] - r[m]) ** 2 + (c[a] - c[m]) ** 2)
                    w = sym * (pv[o] * pv[o]) * np.exp(0.5 * nhl * d2)
                    sp = R2 - 2 - (r[a] + r[m])
                    t = w * tabE[(sp & 1) * R2 + (sp >> 1) + rows]
                    s = hi + t
                    bb = s - hi
                    low = low + ((hi - (s - bb)) + (t - bb))   # (numpy: no FMA for the product's residual)
                    hi = s
            T[tau] = hi + low
        alpha = kinv[o] @ (y[:, o] - pm[o])
        Tm = np.zeros((NP, R))
        Tm[:n] = pv[o] * alpha[:, None] * np.exp(nhl * (rows[None, :] - r[:, None]).astype(np.float64) ** 2)
        # contraction: tabB[par * HB + h] = E(2h + par - (LT - 1)); tabH[v] = H(v - (C - 1))
        t = np.arange(2 * HB)
        par, h = t // HB, t % HB
        tabB = np.exp(0.5 * nhl * (2 * h + par - (LT - 1)).astype(np.float64) ** 2)
        tabH = np.exp(nhl * (np.arange(Cpad + C) - (C - 1)).astype(np.float64) ** 2)
        cols = np.arange(C)
        q = np.zeros((R, C))
        for kb in range(LT // 16):
            B = np.empty((16, C))
            for g in range(4):
                hb = LT // 2 - 1 - 8 * kb - 2 * g
                B[4 * g + 0] = tabB[HB + hb + cols]
                B[4 * g + 1] = tabB[hb + cols]
                B[4 * g + 2] = tabB[HB + hb - 1 + cols]
                B[4 * g + 3] = tabB[hb - 1 + cols]
            q = q + T[16 * kb:16 * kb + 16].T @ B
        cn = np.zeros(NP, dtype=np.int64)
        cn[:n] = c
        m_ = np.zeros((R, C))
        for kb in range(NP // 16):
            k = np.arange(16 * kb, 16 * kb + 16)
            B = tabH[cols[None, :] - cn[k][:, None] + (C - 1)]
            m_ = m_ + Tm[k].T @ B
        mu_o = pm[o] + m_.ravel()
        var_o = np.maximum(pv[o] - q.ravel(), min_var)
        smu = (mu_o - pm[o]) * (1.0 / np.sqrt(pv[o]))
        svar = var_o * (1.0 / pv[o])
        u = smu + betas[o] * np.sqrt(np.abs(svar))
        mu[o], var[o] = mu_o, var_o
        acq = u if o == 0 else acq + u
    return dict(mu=mu, var=var, acq=acq)

"""Model of a tile-to-wave map for the contraction of the grid-convolution path (bo_gridconv.hip,
conv_contract_kernel): which wave tile a wave of a workgroup step takes, and the
k-blocks that the two tiles of a SIMD run, from the band formulas of DESIGN.md §9.4.

A workgroup of W waves takes the W tile slots base .. base + W - 1 per step (base a multiple of W); the kernel
gives wave w the tile base + w (`consecutive`).  `spread` is the candidate that item 7 weighed: when a row
band's cb_n tiles are a multiple of W, the band's cb_n / W steps each take every (cb_n / W)-th tile, so that
waves s and s + W / 2, which share a SIMD, hold tiles cb_n / 2 apart; otherwise the consecutive map."""

import numpy as np

TAB_FLUSH = 2.0 ** -128     # bo_gridconv.hip: kTabFlush


def consecutive(base, wave, W, cb_n):
    return base + wave


def spread(base, wave, W, cb_n):
    if cb_n % W != 0:
        return base + wave
    per = cb_n // W
    step = base // W
    return step // per * cb_n + step % per + wave * per


def bands(C, ls):
    """(hq, hm): the largest |t| whose E(t) = exp(-t^2 / 4 l^2) and H(t) = exp(-t^2 / 2 l^2) are not flushed."""
    LT = -(-(2 * C - 1) // 16) * 16
    nhl = -0.5 / (ls * ls)
    tq, tm = np.arange(LT, dtype=np.float64), np.arange(C, dtype=np.float64)
    return (int(np.flatnonzero(~(np.exp(0.5 * nhl * (tq * tq)) < TAB_FLUSH)).max()),
            int(np.flatnonzero(~(np.exp(nhl * (tm * tm)) < TAB_FLUSH)).max()))


def tile_kblocks(C, n, ls, nb, cstart=None):
    """k-blocks (variance + mean) of each column tile of 16 nb columns, by §9.4; `cstart` is the first row of
    each column's bucket (default: n points spread evenly over the columns)."""
    TW = 16 * nb
    Cpad, LT = -(-C // 64) * 64, -(-(2 * C - 1) // 16) * 16
    hq, hm = bands(C, ls)
    if cstart is None:
        cstart = (np.arange(C + 1) * n) // C
    out = []
    for j0 in range(0, Cpad, TW):
        t_hi = min(2 * (j0 + TW - 1) + hq, LT - 1)
        t_lo = min(2 * j0 - hq, t_hi) if 2 * j0 - hq > 0 else 0
        kq = (t_hi >> 4) + 1 - (t_lo >> 4)
        c_hi = min(j0 + TW + hm, C)
        c_lo = min(j0 - hm, C) if j0 - hm > 0 else 0
        km = max(((int(cstart[c_hi]) + 15) >> 4) - (int(cstart[c_lo]) >> 4), 0)
        out.append(kq + km)
    return np.array(out)


def simd_kblocks(tile_map, row_bands, C, n, ls, nb, W, grid):
    """The k-blocks of every (workgroup, step, SIMD): the sum over the waves s, s + 4, ... of a SIMD (one wave when
    W = 4).  Inactive slots (past the last tile) run the last tile's k-blocks, as the kernel does."""
    cb_n = -(-C // 64) * 64 // (16 * nb)
    n_wt = row_bands * cb_n
    kb = tile_kblocks(C, n, ls, nb)
    out = []
    for b in range(grid):
        for base in range(b * W, n_wt, grid * W):
            tiles = [min(tile_map(base, w, W, cb_n), n_wt - 1) for w in range(W)]
            out.append([sum(kb[tiles[w] % cb_n] for w in range(s, W, 4)) for s in range(min(W, 4))])
    return np.array(out)

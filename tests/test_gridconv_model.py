"""The grid-convolution predict path's arithmetic (bo_gridconv.hip) mirrored in numpy, in the
kernels' accumulation order and table addressing, against the oracle; and the host plan's gate."""

import numpy as np

from oracle import oracle_np as O
from parity import check_predict
import gridconv_model as G


def test_model_matches_oracle_on_a_lattice():
    """37 x 50 grid at grid_lo = (1e6, -7), a 4 x 4 lattice among the training points (midpoints
    shared by many pairs), two objectives with different length scales."""
    shape, lo = (37, 50), (10 ** 6, -7)
    d = G.lattice_problem(shape, lo, 40, 2, seed=5, ls=[1.4, 2.1])
    # the lattice makes midpoints collide: some (tau, sigma) receives several pairs
    r, c = d["rel"][:, 0], d["rel"][:, 1]
    iu = np.triu_indices(40)
    mids = np.stack([(r[:, None] + r[None, :])[iu], (c[:, None] + c[None, :])[iu]], axis=1)
    assert np.unique(mids, axis=0, return_counts=True)[1].max() >= 3
    got = G.model_predict(d["x"], d["y"], d["Kinv"], d["pm"], d["pv"], d["ls"], d["betas"], shape, lo)
    ref = O.predict_acquire(d["x"], d["y"], G.grid_points(shape, lo), d["pm"], d["pv"], d["ls"], d["betas"],
                            kinv=d["Kinv"])
    check_predict(got, {k: ref[k] for k in ("mu", "var", "acq")}, d["pv"])
    # far inside the rule: the regrouped sum's error is the quadratic form's own rounding
    assert np.abs(got["var"] - ref["var"]).max() <= 1e-9 * d["pv"].max()


def test_plan_gate():
    # the headline (C3) and C2 take the new path; so do the small grids once forced
    assert G.conv_planned((1024, 1024), 512, 2)
    assert G.conv_planned((512, 512), 128, 2)
    assert G.conv_planned((37, 50), 8, 2, mode="auto-conv")
    # few training points on a wide grid: the chunk-major kernel is cheaper
    assert not G.conv_planned((1024, 1024), 32, 2)
    assert not G.conv_planned((37, 500), 8, 2)
    assert G.conv_planned((37, 500), 8, 2, mode="auto-conv")
    # never: other modes, other dimensions, tables beyond the LDS, N beyond the setup kernel's cap
    for mode in ("dense", "auto-exp", "dense-exp", "fp32", "auto-noconv"):
        assert not G.conv_planned((1024, 1024), 512, 2, mode=mode)
    assert not G.conv_planned((4, 8, 64), 150, 2)
    assert not G.conv_planned((64, 8192), 512, 2, mode="auto-conv")
    assert not G.conv_planned((8192, 64), 512, 2, mode="auto-conv")
    assert not G.conv_planned((64, 64), 4097, 2, mode="auto-conv")
    # a shard of a few candidates pays the pair stage of its whole rows
    assert not G.conv_planned((1024, 1024), 512, 2, offset=5, count=16)


# measured on MI355X (profiles/gridconv_crossover.json): (side, N, new path us, chunk-major us)
CROSSOVER = [(64, 32, 69.1, 25.9), (64, 64, 94.2, 28.8), (64, 128, 187.4, 38.6), (64, 256, 547.8, 63.4),
             (64, 512, 2302.6, 158.5), (256, 32, 87.3, 37.6), (256, 64, 98.5, 46.7), (256, 128, 135.1, 77.1),
             (256, 256, 233.4, 185.3), (256, 512, 657.4, 551.2), (1024, 32, 203.4, 182.9),
             (1024, 64, 208.4, 314.6), (1024, 128, 226.7, 739.6), (1024, 256, 284.2, 2520.9),
             (1024, 512, 454.7, 8351.2)]


def test_gate_follows_the_measured_crossover():
    """The gate's time model against the measured table: it never plans the new path where that
    measured slower, plans it wherever it measured 1.3x faster or more, and both modelled times
    are within 35 % of the measured ones (the fit is within 20 %; the margin covers it)."""
    for side, n, conv_us, old_us in CROSSOVER:
        planned = G.conv_planned((side, side), n, 2)
        if conv_us > old_us:
            assert not planned, (side, n)
        if old_us > 1.3 * conv_us:
            assert planned, (side, n)
        m_conv, m_old = G.gate_times((side, side), n, 2)
        assert abs(m_conv / conv_us - 1) < 0.35 and abs(m_old / old_us - 1) < 0.35, (side, n, m_conv, m_old)

"""numpy model of the contraction's top-q lists (bo_predict.hip plan_gridconv, bo_gridconv.hip): a workgroup
of the contraction merges its waves' lists and writes one, and the plan launches no more workgroups than the
final merge reads lists (n_lists = the chunk-major kernel's grid x its 4 waves, the partial-list buffer's
layout, which the tile width must not change) -- for every tile width, forced or chosen, on the tabulated
descriptors of profiles/layout_workspace_sizes.txt and a random few thousand."""

import os

import numpy as np

K_WAVES, K_TILE = 4, 64          # bo_predict.hip: waves of a chunk-major workgroup, candidates of its tile
BUFFER_LISTS = 1024 * K_WAVES    # make_plan: the partial lists are sized for the largest persistent grid
MAX_TOPQ = 48


def n_lists(count, cus, small):
    slots = 2 * cus if small else cus
    return K_WAVES * min(max(-(-count // K_TILE), 1), slots)


def choose_nb(tiles64, cus):
    """plan_gridconv: the widest tile that still gives every SIMD two."""
    return 4 if tiles64 >= 8 * cus else 2 if 2 * tiles64 >= 8 * cus else 1


def contraction(R, C, offset, count, cus, small, forced=None):
    """(nb, waves per workgroup, workgroups = lists written)."""
    row_lo = offset // C
    nrows = (offset + count - 1) // C - row_lo + 1
    ldr, Cpad = -(-nrows // 16) * 16, -(-C // 64) * 64
    tiles64 = (ldr // 16) * (Cpad // 64)
    nb = forced or choose_nb(tiles64, cus)
    tiles = tiles64 * (4 // nb)
    waves = 8 if tiles >= 8 * cus else 4
    wgs = min(-(-tiles // waves), cus, n_lists(count, cus, small))
    return nb, waves, wgs


def _tabulated():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                        "layout_workspace_sizes.txt")
    out = []
    with open(path) as f:
        for line in f:
            t = line.split()
            if len(t) >= 8 and t[0].isdigit():
                R, C = int(t[0]), int(t[1])
                offset = int(t[6])
                count = R * C - offset if t[7] == "all" else int(t[7])
                out.append((R, C, int(t[4]), offset, count))
    return out


def _check(R, C, q, offset, count):
    for cus in (64, 104, 228, 256, 304):
        for small in (False, True):
            nl = n_lists(count, cus, small)
            assert 1 <= nl <= BUFFER_LISTS
            for forced in (None, 1, 2, 4):
                nb, waves, wgs = contraction(R, C, offset, count, cus, small, forced)
                assert nb in (1, 2, 4) and waves in (4, 8)
                assert 1 <= wgs <= nl, (R, C, offset, count, cus, forced)
                assert wgs <= cus                                  # one resident workgroup per CU
                assert waves * max(q, 1) * 16 <= 8 * MAX_TOPQ * 16  # the merge's LDS: at most 6 KiB


def test_tabulated_descriptors():
    rows = _tabulated()
    assert len(rows) == 76
    for R, C, q, offset, count in rows:
        _check(R, C, q, offset, count)


def test_headline_shapes():
    """C3 (1024 x 1024) takes 32-column tiles on 8-wave workgroups, one per CU; C2 (512 x 512) 16-column tiles
    on 4-wave workgroups, a wave on every SIMD."""
    assert contraction(1024, 1024, 0, 1024 * 1024, 256, False) == (2, 8, 256)
    assert contraction(512, 512, 0, 512 * 512, 256, True) == (1, 4, 256)
    assert contraction(1024, 1024, 0, 1024 * 1024, 256, False, forced=4) == (4, 4, 256)


def test_random_descriptors():
    rng = np.random.default_rng(7)
    for _ in range(4000):
        R, C = int(rng.integers(1, 5001)), int(rng.integers(1, 3601))
        total = R * C
        if rng.random() < 0.5:
            offset, count = 0, total
        else:
            offset = int(rng.integers(0, total))
            count = int(rng.integers(1, total - offset + 1))
            if rng.random() < 0.3:
                count = min(count, int(rng.integers(1, 300)))     # shards of a few candidates: few lists
        _check(R, C, int(rng.integers(0, MAX_TOPQ + 1)), offset, count)

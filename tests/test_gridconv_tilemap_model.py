"""The tile-to-wave maps of tests/gridconv_tilemap_model.py: the spread map is a permutation of the wave tiles
that keeps a workgroup step inside one row band and puts the two tiles of a SIMD into different halves of the
row, and what it does to the k-blocks per SIMD at the headline shapes."""

import numpy as np
import pytest

import gridconv_tilemap_model as M

# (row bands, cb_n, W, grid): cb_n a multiple of W and not, a grid smaller and larger than the tile groups, one band
SWEEP = [(rb, cb_n, W, grid)
         for rb in (1, 2, 5, 64)
         for cb_n in (4, 8, 12, 16, 20, 32, 36, 64, 128)
         for W in (4, 8)
         for grid in (1, 3, 16, 256, 1000)]


@pytest.mark.parametrize("tile_map", [M.consecutive, M.spread])
def test_bijection_and_one_row_band_per_step(tile_map):
    for rb, cb_n, W, grid in SWEEP:
        n_wt = rb * cb_n
        seen = np.zeros(n_wt, dtype=np.int64)
        for b in range(min(grid, -(-n_wt // W))):
            for base in range(b * W, n_wt, grid * W):
                tiles = [tile_map(base, w, W, cb_n) for w in range(W)]
                live = [t for t in tiles if t < n_wt]
                assert all(t >= 0 for t in tiles)
                np.add.at(seen, live, 1)
                if cb_n % W == 0:
                    assert len(live) == W and len({t // cb_n for t in live}) == 1, (rb, cb_n, W, grid, base)
        assert (seen == 1).all(), (rb, cb_n, W, grid)


def test_spread_separates_the_two_tiles_of_a_simd():
    for rb, cb_n, W, grid in SWEEP:
        if cb_n % W != 0:
            # the general case is the consecutive map
            assert all(M.spread(base, w, W, cb_n) == base + w for base in range(0, rb * cb_n, W) for w in range(W))
            continue
        for base in range(0, rb * cb_n, W):
            cols = [M.spread(base, w, W, cb_n) % cb_n for w in range(W)]
            assert np.diff(cols).tolist() == [cb_n // W] * (W - 1)
            for s in range(W // 2):
                assert cols[s] * 4 // cb_n != cols[s + W // 2] * 4 // cb_n        # not the same quarter of the row


def test_c3_and_c2_kblocks_per_simd():
    """C3 (1024 x 1024, N = 512, 32-column tiles, 8 waves): the longest SIMD under the spread map is not longer
    than under the consecutive one -- and barely shorter (142 -> 139 k-blocks): 20 of a row's 32 tiles run the
    full band, so some SIMD of EVERY workgroup still holds two of them, where the consecutive map gives that
    to the centre workgroups only.  C2 (one wave per SIMD): the map moves no maximum."""
    c3 = [M.simd_kblocks(f, 64, 1024, 512, 20.0, 2, 8, 256) for f in (M.consecutive, M.spread)]
    assert c3[0].sum() == c3[1].sum()
    assert c3[1].max() <= c3[0].max()
    assert (c3[0].max(), c3[1].max()) == (142, 139)
    assert c3[1].max(axis=1).min() == c3[1].max()          # every workgroup has a SIMD as long as the longest
    c2 = [M.simd_kblocks(f, 32, 512, 128, 20.0, 1, 4, 256) for f in (M.consecutive, M.spread)]
    assert c2[0].max() == c2[1].max() == 58

"""The closed form of the pair list's offsets and the class function of the accumulate kernel's work
order (gridconv_sched_model.py, the numpy statement of what bo_gridconv.hip computes), against brute
force."""

import numpy as np
import pytest

import gridconv_sched_model as S


def _lt(C):
    return -(-(2 * C - 1) // 16) * 16


def _designs():
    rng = np.random.default_rng(7)
    out = {}
    for i, (C, n) in enumerate(((23, 40), (64, 300), (45, 7), (300, 512), (1024, 512))):
        out[f"random-{C}-{n}"] = (C, rng.integers(0, C, size=n))
    out["one-column"] = (17, np.full(40, 5))
    out["one-per-column"] = (33, rng.permutation(33))
    out["edges"] = (45, np.array([0, 0, 44, 44]))              # tau = 0 and tau = 2C - 2
    out["neighbours"] = (45, np.array([7, 8, 8, 20, 21]))      # odd tau
    out["single"] = (45, np.array([13]))
    out["clustered"] = (256, 100 + rng.integers(0, 40, size=300))
    return out


_DESIGNS = _designs()


@pytest.mark.parametrize("name", sorted(_DESIGNS))
def test_pstart_closed_form(name):
    C, cols = _DESIGNS[name]
    LT = _lt(C)
    got, want = S.pstart_closed(cols, C, LT), S.pstart_brute(cols, C, LT)
    np.testing.assert_array_equal(got, want)
    n = len(cols)
    assert got[0] == 0 and (got[2 * C - 1:] == n * (n + 1) // 2).all()      # the padding tau are empty


def test_pstart_edge_counts():
    C, cols = _DESIGNS["edges"]
    cnt = np.diff(S.pstart_closed(cols, C, _lt(C)))
    assert cnt[0] == 3 and cnt[2 * C - 2] == 3 and cnt[C - 1] == 4 and cnt.sum() == 10
    C, cols = _DESIGNS["neighbours"]
    cnt = np.diff(S.pstart_closed(cols, C, _lt(C)))
    assert cnt[15] == 2 and cnt[41] == 1 and cnt[16] == 3


def test_pair_class_values():
    assert [S.pair_class(k) for k in (1, 2, 3, 4, 6)] == [0, 2, 3, 4, 5]
    assert S.pair_class(2 ** 16) == 32 and S.pair_class(2 ** 16 * 3 // 2) == 33
    assert S.pair_class(4096 * 4097 // 2) < 48                 # the longest list of n <= 4096


def test_pair_class_monotone_and_narrow():
    ks = np.unique(np.concatenate([np.arange(1, 5000), (2.0 ** np.arange(12, 24, 0.25)).astype(np.int64),
                                   2 ** np.arange(1, 24) - 1, 2 ** np.arange(1, 24) + 1]))
    cls = np.array([S.pair_class(k) for k in ks])
    assert (np.diff(cls) >= 0).all()
    # a class spans a factor below 2: its lists are [2^e, 1.5 2^e) or [1.5 2^e, 2^(e+1))
    for c in np.unique(cls):
        e, half = divmod(int(c), 2)
        lo = 2 ** e + (2 ** e // 2 if half else 0)
        hi = 2 ** e + 2 ** e // 2 if half == 0 and e > 0 else 2 ** (e + 1)
        assert S.pair_class(lo) == c and S.pair_class(hi - 1) == c and S.pair_class(hi) > c
        assert hi - 1 < 2 * lo
        members = ks[cls == c]
        assert members.min() >= lo and members.max() < hi

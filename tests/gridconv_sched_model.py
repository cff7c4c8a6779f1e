"""numpy statement of the pair stage's schedule (bayesopt_smart_amd/csrc/bo_gridconv.hip): the offset
of a tau's pairs in the pair list, which conv_list_kernel computes from the column buckets alone, and
the class of a tau's kept pair count, by which conv_acc_kernel orders its work."""

import numpy as np


def pstart_closed(cols, C, LT):
    """pstart[t], t = 0 .. LT: the pairs n <= m with c_n + c_m < t.  With h[c] the points of column c
    and cum(x) = cstart[clamp(x, 0, C)], the ordered pairs are sum_c h[c] cum(t - c); the n = m among
    them (2 c_n < t, cum(ceil(t / 2)) of them) were counted once and every other pair twice."""
    cols = np.asarray(cols, dtype=np.int64)
    h = np.bincount(cols, minlength=C)
    cstart = np.concatenate([[0], np.cumsum(h)])
    t = np.arange(LT + 1)
    c = np.arange(C)
    ordered = (h[None, :] * cstart[np.clip(t[:, None] - c[None, :], 0, C)]).sum(axis=1)
    return (ordered + cstart[np.minimum((t + 1) // 2, C)]) // 2


def pstart_brute(cols, C, LT):
    """The same by counting: an exclusive cumulative sum of the pairs per tau."""
    cols = np.asarray(cols, dtype=np.int64)
    iu = np.triu_indices(cols.size)
    cnt = np.bincount(cols[iu[0]] + cols[iu[1]], minlength=LT)
    return np.concatenate([[0], np.cumsum(cnt)])


def pair_class(k):
    """Class of a list of k >= 1 pairs: 2 floor(log2 k) + the bit below the leading one (half-octaves)."""
    k = int(k)
    assert k >= 1
    e = k.bit_length() - 1
    return 2 * e + ((k >> (e - 1)) & 1 if e > 0 else 0)

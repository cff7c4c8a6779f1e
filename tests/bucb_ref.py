"""numpy reference of the hallucinated-observation batch (GP-BUCB) for tests/test_gpu_bucb.py.

Independent of the device formulation: the variance after t picks is the posterior variance of a
GP trained on X u {p_1..p_t}, computed by inverting the augmented Gram matrix (jitter on every
point) from scratch at every step -- no recursion, no weight vectors.
"""
import numpy as np

RTOL = 1e-5                     # tests/parity.py's rule: var 1e-5 pv, acq 1e-5 max(1, |ref|)


def rbf(a, b, pv, ls):
    d = a[:, None, :] - b[None, :, :]
    return pv * np.exp(-0.5 * np.einsum("ijk,ijk->ij", d, d) / (ls * ls))


def fitted_state(x, y, pm, pv, ls, jitter):
    """kinv [n_obj, N, N] = inv(K_o + jitter I) and cond(K_o + jitter I) per objective."""
    n_obj = len(pv)
    kinv = np.empty((n_obj, x.shape[0], x.shape[0]))
    cond = np.empty(n_obj)
    for o in range(n_obj):
        k = rbf(x, x, pv[o], ls[o]) + jitter * np.eye(x.shape[0])
        kinv[o] = np.linalg.inv(k)
        cond[o] = np.linalg.cond(k)
    return kinv, cond


def posterior(x, y, cand, pm, pv, ls, jitter, min_var, extra=None):
    """std_mu, var [n_obj, M] of the GP on x (mean from y); `extra` (points [t, d]): the variance
    of the GP on x u extra instead (the mean is not conditioned on them)."""
    n_obj = len(pv)
    smu = np.empty((n_obj, cand.shape[0]))
    var = np.empty_like(smu)
    xa = x if extra is None or len(extra) == 0 else np.concatenate([x, extra])
    for o in range(n_obj):
        ks = rbf(cand, x, pv[o], ls[o])
        kinv = np.linalg.inv(rbf(x, x, pv[o], ls[o]) + jitter * np.eye(x.shape[0]))
        smu[o] = ks @ (kinv @ (y[:, o] - pm[o])) / np.sqrt(pv[o])
        ka = rbf(cand, xa, pv[o], ls[o])
        kainv = np.linalg.inv(rbf(xa, xa, pv[o], ls[o]) + jitter * np.eye(xa.shape[0]))
        var[o] = np.maximum(pv[o] - np.einsum("ij,jk,ik->i", ka, kainv, ka), min_var)
    return smu, var


def acquisition(smu, var, pv, beta):
    pv = np.asarray(pv)[:, None]
    return (smu + np.asarray(beta)[:, None] * np.sqrt(np.abs(var) / pv)).sum(axis=0)


def best(acq, avail):
    """Index of the best available candidate in select_next_batch's order (NaN first, descending
    value, ascending index), -1 when none is left; and the gap to the second best."""
    idx = np.flatnonzero(avail)
    if idx.size == 0:
        return -1, np.inf
    a = acq[idx]
    key = np.where(np.isnan(a), np.inf, a)
    order = np.argsort(-key, kind="stable")
    gap = key[order[0]] - key[order[1]] if idx.size > 1 else np.inf
    return int(idx[order[0]]), float(gap)


def bucb_reference(x, y, cand, pm, pv, ls, beta, jitter, min_var, q, excluded, picks=None):
    """The batch over `cand` (the shard's points, local indices).  Returns a dict: idx [q] (local,
    -1 = none left), val [q], gaps [q] (best-to-second gap of acq_t), var (after all picks), acq
    (the acquisition the last pick was taken from), smu / var0 (the inputs of the device call).
    `picks`: take these local indices instead of the arg-max (conditioning on the device's own
    choice)."""
    smu, var0 = posterior(x, y, cand, pm, pv, ls, jitter, min_var)
    avail = ~np.asarray(excluded, dtype=bool)
    var = var0
    idx, val, gaps = [], [], []
    acq = None
    for t in range(q):
        acq = acquisition(smu, var, pv, beta)
        p, gap = best(acq, avail)
        if picks is not None:
            p = int(picks[t])
        idx.append(p)
        val.append(acq[p] if p >= 0 else -np.inf)
        gaps.append(gap)
        if p >= 0:
            avail[p] = False
            chosen = cand[[i for i in idx if i >= 0]]
            _, var = posterior(x, y, cand, pm, pv, ls, jitter, min_var, extra=chosen)
    return {"idx": np.array(idx), "val": np.array(val), "gaps": np.array(gaps), "var": var, "acq": acq,
            "smu": smu, "var0": var0}

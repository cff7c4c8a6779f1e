"""numpy reference of the Kriging-believer batch for the EHVI (tests/test_gpu_kb.py, tests/test_kb_api.py).

Independent of the device's formulation and of its form: the variance after t picks is the posterior
variance of a GP trained on X u {p_1..p_t}, from the inverse of the augmented Gram matrix
(bucb_ref.posterior(..., extra=picks): no recursion, no weight vectors); the EHVI is ehvi_ref.ehvi,
the textbook closed form per box; the boxes are the library's host decomposition
(acquisition.hypervolume_boxes) of the front extended by the believed means; the selection is
bucb_ref.best (NaN first, descending value, ascending index).
"""
import numpy as np

import bucb_ref as B
import ehvi_ref as E

RTOL = B.RTOL                   # tests/parity.py's rule: var 1e-5 pv, acq 1e-5 max(1, |ref|)


def pareto_front(y):
    """Rows of y no other row dominates (maximisation)."""
    y = np.asarray(y, dtype=np.float64)
    ge = (y[:, None, :] >= y[None, :, :]).all(-1)
    gt = (y[:, None, :] > y[None, :, :]).any(-1)
    return y[~(ge & gt).any(axis=0)]


def objective_posterior(x, y, cand, pm, pv, ls, jitter, min_var):
    """mu, var [n_obj, M] in objective units: the inputs of the device call."""
    smu, var = B.posterior(x, y, cand, pm, pv, ls, jitter, min_var)
    return np.asarray(pm)[:, None] + np.sqrt(np.asarray(pv))[:, None] * smu, var


def kb_reference(x, y, cand, pm, pv, ls, jitter, min_var, q, excluded, front, ref_point, picks=None, mu=None):
    """The batch over `cand` (the shard's points, local indices).  Returns a dict: idx [q] (local,
    -1 = none left), val [q], gaps [q] (best-to-second gap of acq_t), var (after all q picks),
    acq_first / acq_last, believed [q, n_obj] (NaN rows where no candidate was left), n_boxes (per
    pick), mu / var0 (the inputs of the device call).  `picks`: follow these local indices instead
    of the arg-max; `mu`: this mean instead of the posterior's (e.g. with a NaN put in)."""
    from bayesopt_smart_amd.acquisition import hypervolume_boxes
    mu0, var0 = objective_posterior(x, y, cand, pm, pv, ls, jitter, min_var)
    mu = mu0 if mu is None else np.asarray(mu, dtype=np.float64)
    n_obj = mu.shape[0]
    ref_point = np.asarray(ref_point, dtype=np.float64)
    cur = np.asarray(front, dtype=np.float64).reshape(-1, n_obj)
    avail = ~np.asarray(excluded, dtype=bool)
    var = var0
    idx, val, gaps, believed, n_boxes = [], [], [], [], []
    acq_first = acq = None
    for t in range(q):
        boxes = hypervolume_boxes(cur, ref_point)
        n_boxes.append(boxes.shape[0])
        acq = E.ehvi(mu, var, boxes)
        if t == 0:
            acq_first = acq
        p, gap = B.best(acq, avail)
        if picks is not None:
            p = int(picks[t])
        idx.append(p)
        val.append(acq[p] if p >= 0 else -np.inf)
        gaps.append(gap)
        believed.append(mu[:, p].copy() if p >= 0 else np.full(n_obj, np.nan))
        if p >= 0:
            avail[p] = False
            cur = np.concatenate([cur, mu[:, p][None, :]])
            chosen = cand[[i for i in idx if i >= 0]]
            _, var = B.posterior(x, y, cand, pm, pv, ls, jitter, min_var, extra=chosen)
    return {"idx": np.array(idx), "val": np.array(val), "gaps": np.array(gaps), "var": var, "acq_first": acq_first,
            "acq_last": acq, "believed": np.array(believed), "n_boxes": np.array(n_boxes), "mu": mu, "var0": var0}

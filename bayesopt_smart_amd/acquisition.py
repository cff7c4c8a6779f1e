"""Drop-in mirror of bayesopt/acquisition.py on the MI355X (same names and semantics).

Arrays may be numpy (results copied back in place, as the reference mutates them) or HIP
device tensors.
"""

from __future__ import annotations

import ctypes as _C

import numpy as np
import torch

from . import _lib
from .device import F64, Workspace, require_device, stream_handle
from .kernels import _Arg, _dev_of, _host_vec

C_i64 = _C.c_int64


def upper_confidence_bound(mu, variance, beta):
    """acquisition.py:33-52 — mu + beta * sqrt(|variance|) (returns a new array)."""
    dev = _dev_of(mu, variance)
    m = _Arg(mu, dev)
    v = _Arg(variance, dev)
    out = torch.empty_like(m.t)
    _lib.check(_lib.load().bo_update_ucb(out.data_ptr(), m.ptr, v.ptr, 1, m.t.numel(),
                                         _host_vec([beta], 1), stream_handle(dev)), "bo_update_ucb")
    return out if isinstance(mu, torch.Tensor) else out.cpu().numpy()


def update_ucb(ucb, mu_objectives, variance_objectives, betas):
    """acquisition.py:55-81 — per-objective UCB, in place."""
    dev = _dev_of(ucb, mu_objectives)
    u = _Arg(ucb, dev, write=True)
    m = _Arg(mu_objectives, dev)
    v = _Arg(variance_objectives, dev)
    n_obj, n = m.t.shape
    _lib.check(_lib.load().bo_update_ucb(u.ptr, m.ptr, v.ptr, n_obj, n, _host_vec(betas, n_obj),
                                         stream_handle(dev)), "bo_update_ucb")
    u.finish()


def update_hypervolume_improvement(acquisition_values, ucb):
    """acquisition.py:89-108 — the reference's "HVI": sum of per-objective UCB, in place."""
    dev = _dev_of(acquisition_values, ucb)
    a = _Arg(acquisition_values, dev, write=True)
    u = _Arg(ucb, dev)
    n_obj, n = u.t.shape
    _lib.check(_lib.load().bo_update_hypervolume_improvement(a.ptr, u.ptr, n_obj, n, stream_handle(dev)),
               "bo_update_hypervolume_improvement")
    a.finish()


def _grid_args(cands):
    lo = (C_i64 * 8)(*(list(cands.lo or []) + [0] * (8 - len(cands.lo or []))))
    sh = (C_i64 * 8)(*(list(cands.shape or []) + [1] * (8 - len(cands.shape or []))))
    return lo, sh


class ExclusionMask:
    """The exclusion of acquisition.py:137-139 -- a candidate equal in every coordinate to an
    evaluated point is never selected -- as a device bit mask over one candidate shard
    ([offset, offset + count) of `cands`), kept across iterations (bo_excl_mask_update).

    The loop's evaluated set only grows (x_vector[:n], the new batch appended each iteration),
    so `update(points)` adds the rows it has not seen yet: one thread per new point on a grid,
    one pass over the shard otherwise.  A shorter or changed prefix rebuilds the mask.  The
    masked selections (bo_select_topq_masked, bo_hvi_select_topq_masked) then drop an excluded
    element as they load it: no per-call hash set and no probes."""

    def __init__(self, cands, offset=0, count=None, device=None):
        self.cands = cands
        self.offset = int(offset)
        self.count = int(cands.n - offset if count is None else count)
        self.dev = require_device(device)
        lib = _lib.load()
        self.bits = torch.zeros(lib.bo_excl_mask_bytes(self.count) // 4, dtype=torch.int32, device=self.dev)
        self.n_seen = 0
        self._seen = None              # host copy of the rows already in the mask

    @property
    def ptr(self):
        return self.bits.data_ptr()

    def update(self, evaluated_points):
        ev = np.ascontiguousarray(np.asarray(evaluated_points.cpu().numpy() if isinstance(evaluated_points, torch.Tensor)
                                             else evaluated_points, dtype=np.float64).reshape(-1, self.cands.dim))
        n = ev.shape[0]
        clear = n < self.n_seen or (self.n_seen > 0 and not np.array_equal(ev[: self.n_seen], self._seen))
        first = 0 if clear else self.n_seen
        if first == n and not clear:
            return self
        lib = _lib.load()
        ex = torch.as_tensor(ev, device=self.dev)
        ws = Workspace.get(lib.bo_excl_mask_workspace_size(n - first), self.dev)
        lo, sh = _grid_args(self.cands)
        carg = self.cands.cand_arg
        if self.cands.kind in ("i64", "f64"):
            carg = self.cands.tensor[self.offset:].data_ptr()
        _lib.check(lib.bo_excl_mask_update(self.ptr, self.count, self.cands.kind_code, carg, lo, sh,
                                           self.cands.dim, self.offset, ex.data_ptr() if n else None, first, n,
                                           1 if clear else 0, ws.data_ptr(), ws.numel(),
                                           stream_handle(self.dev)), "bo_excl_mask_update")
        self._keep = ex                # the points stay alive until the stream has used them
        self.n_seen = n
        self._seen = ev.copy()
        return self

    def excluded(self):
        """Host bool array [count]: the candidates the mask excludes."""
        w = self.bits.cpu().numpy().view(np.uint32)
        return np.unpackbits(w.view(np.uint8), bitorder="little")[: self.count].astype(bool)


def _shard_mask(mask, cands, offset, count, dev, evaluated_points, who):
    """The ExclusionMask of the shard [offset, offset + count) of `cands`, updated with
    evaluated_points: `mask` when it covers that shard (else `who` raises), a new one without."""
    if mask is None:
        mask = ExclusionMask(cands, offset, count, dev)
    elif mask.offset != offset or mask.count != count:
        raise ValueError(f"{who}: the mask covers another shard")
    return mask.update(evaluated_points)


def _set_cand_fields(d, cands, offset, count):
    """The shard [offset, offset + count) of `cands` into a descriptor's candidate fields (the ones
    bo_bucb_desc, bo_kb_desc and bo_ts_desc share)."""
    d.dim, d.cand_kind = cands.dim, cands.kind_code
    d.n_cand, d.cand_offset = count, offset
    if cands.kind == "grid":
        for k in range(cands.dim):
            d.grid_lo[k] = cands.lo[k]
            d.grid_shape[k] = cands.shape[k]
    elif cands.kind == "sobol":
        d.cand = cands.cand_arg
    else:                                              # explicit candidates: the shard's rows
        d.cand = cands.tensor.data_ptr() + offset * cands.dim * cands.tensor.element_size()


def _fitted_ok(x, kinv, dim, n_obj):
    """x is [N, dim] and kinv [n_obj, >= N, >= N] (square)."""
    return x.dim() == 2 and x.shape[1] == dim and kinv.dim() == 3 and kinv.shape[0] == n_obj \
        and kinv.shape[1] == kinv.shape[2] and kinv.shape[1] >= x.shape[0]


def _record_indices(rec, q):
    """The valid global indices of a device record block [2 q] (values, bit-cast int64 indices)."""
    idx = rec[q:].view(torch.int64).cpu().numpy()
    return idx[idx >= 0]


def check_constraint_bounds(constraint_bounds, n_constraints=None):
    """The outcome constraints' bounds as a float64 array [n_con, 2] (lo, hi), checked by the rules of
    bo_constrained_ehvi: lo <= hi, neither NaN, each infinite on its own side only."""
    b = np.asarray([] if constraint_bounds is None else constraint_bounds, dtype=np.float64).reshape(-1, 2)
    if n_constraints is not None and b.shape[0] != n_constraints:
        raise ValueError(f"constraint_bounds must hold one (lo, hi) pair per constraint: got {b.shape[0]} "
                         f"for n_constraints={n_constraints}")
    for j, (lo, hi) in enumerate(b):
        if np.isnan(lo) or np.isnan(hi):
            raise ValueError(f"constraint {j}: a bound is NaN (use -inf / +inf for a one-sided constraint)")
        if lo > hi:
            raise ValueError(f"constraint {j}: the lower bound {lo} exceeds the upper bound {hi}: no value is feasible")
        if lo == np.inf or hi == -np.inf:
            raise ValueError(f"constraint {j}: lo = +inf or hi = -inf leaves no feasible value")
    return b


def feasible_rows(y, n_obj, constraint_bounds):
    """Host bool array [len(y)]: the rows of y ([n, n_obj + n_con], objectives first) whose constraint
    outputs all lie inside their bounds, lo_j <= y[:, n_obj + j] <= hi_j (a NaN output is infeasible).
    The one statement of feasibility: the loop's front and pareto_analysis both use it."""
    y = np.asarray(y.cpu().numpy() if isinstance(y, torch.Tensor) else y, dtype=np.float64)
    b = check_constraint_bounds(constraint_bounds)
    y = y.reshape(-1, n_obj + b.shape[0])
    g = y[:, n_obj:]
    return np.all((g >= b[:, 0]) & (g <= b[:, 1]), axis=1)


def _front_of(y_vector, n_evaluations, reference_point, constraint_bounds=None):
    """The Pareto-efficient rows (device filter, pareto.py:12-45) of y_vector[:n_evaluations], host.
    With constraint_bounds: of the feasible rows only (feasible_rows), over the objective columns
    (the first len(reference_point)) only."""
    from .pareto import is_pareto_efficient
    y = y_vector[:n_evaluations]
    if constraint_bounds is not None:
        n_obj = len(reference_point)
        y = np.asarray(y.cpu().numpy() if isinstance(y, torch.Tensor) else y)
        y = np.ascontiguousarray(y[feasible_rows(y, n_obj, constraint_bounds)][:, :n_obj])
        n_evaluations = y.shape[0]
    front = y[is_pareto_efficient(y)] if n_evaluations > 0 else np.zeros((0, len(reference_point)))
    return front.cpu().numpy() if isinstance(front, torch.Tensor) else front


def select_indices(acquisition_values, cands, evaluated_points, batch_size, dev=None, mask=None):
    """Global candidate indices of select_next_batch's choice (device top-q with exclusion).

    Order: NaN first, then descending value, ties by ascending index (the reference's
    argsort tie order is unspecified).  Batches above BO_MAX_TOPQ are taken in rounds,
    each round excluding the points already chosen.  `mask` (an ExclusionMask of the whole set,
    already updated with evaluated_points) replaces the per-call exclusion when the batch fits
    one call.
    """
    dev = dev or _dev_of(acquisition_values, evaluated_points)
    acq = _Arg(acquisition_values, dev)
    lib = _lib.load()
    if mask is not None and batch_size <= _lib.MAX_TOPQ:
        tv = torch.empty(batch_size, dtype=F64, device=dev)
        ti = torch.empty(batch_size, dtype=torch.int64, device=dev)
        ws = Workspace.get(lib.bo_select_topq_workspace_size(cands.n, batch_size), dev)
        _lib.check(lib.bo_select_topq_masked(acq.ptr, cands.n, 0, mask.ptr, batch_size, tv.data_ptr(),
                                             ti.data_ptr(), ws.data_ptr(), ws.numel(), stream_handle(dev)),
                   "bo_select_topq_masked")
        got = ti.cpu().numpy()
        return got[got >= 0].astype(np.int64)
    ev = np.asarray(evaluated_points.cpu().numpy() if isinstance(evaluated_points, torch.Tensor)
                    else evaluated_points, dtype=np.float64).reshape(-1, cands.dim)
    chosen = []
    while len(chosen) < batch_size:
        q = min(_lib.MAX_TOPQ, batch_size - len(chosen))
        excl = ev if not chosen else np.concatenate([ev, cands.points(np.array(chosen)).astype(np.float64)])
        ex = torch.as_tensor(np.ascontiguousarray(excl), device=dev)
        tv = torch.empty(q, dtype=F64, device=dev)
        ti = torch.empty(q, dtype=torch.int64, device=dev)
        lo, sh = _grid_args(cands)
        nbytes = lib.bo_select_topq_workspace_size(cands.n, q)
        ws = Workspace.get(nbytes, dev)
        _lib.check(lib.bo_select_topq(acq.ptr, cands.n, cands.kind_code, cands.cand_arg, lo, sh, cands.dim, 0, ex.data_ptr() if ex.numel() else None,
                                      ex.shape[0], q, tv.data_ptr(), ti.data_ptr(), ws.data_ptr(),
                                      ws.numel(), stream_handle(dev)), "bo_select_topq")
        got = [int(i) for i in ti.cpu().numpy() if i >= 0]
        chosen.extend(got)
        if len(got) < q:
            break
    return np.array(chosen, dtype=np.int64)


def select_next_batch(input_space, acquisition_values, evaluated_points, batch_size=3):
    """acquisition.py:116-144 — the best `batch_size` candidates (descending acquisition)
    that are not equal to an evaluated point; returns a new array of candidate rows."""
    from .predict import CandidateSet
    cands = CandidateSet.explicit(input_space, _dev_of(acquisition_values, input_space))
    idx = select_indices(acquisition_values, cands, evaluated_points, batch_size)
    if isinstance(input_space, torch.Tensor):
        return input_space[torch.as_tensor(idx, device=input_space.device)].cpu().numpy()
    return np.asarray(input_space)[idx]



# ------------------------------------------------------- exact hypervolume improvement
def hypervolume_boxes(front, reference_point) -> np.ndarray:
    """Disjoint boxes [lower, upper) (rows of 2*n_obj, upper may be +inf) covering the region
    above `reference_point` that no row of `front` dominates (maximisation); host decomposition
    in the library (bo_hvi_boxes).  Not in the reference (its reference point is unused,
    bayesian_optimization.py:65)."""
    f = np.ascontiguousarray(np.asarray(front.cpu().numpy() if isinstance(front, torch.Tensor) else front,
                                        dtype=np.float64))
    r = np.ascontiguousarray(np.asarray(reference_point, dtype=np.float64).ravel())
    n_obj = r.size
    f = f.reshape(-1, n_obj)
    lib = _lib.load()
    cnt = C_i64(0)
    dp = _C.POINTER(_C.c_double)
    cap = 1024
    while True:
        out = np.empty((cap, 2 * n_obj), dtype=np.float64)
        st = lib.bo_hvi_boxes(f.ctypes.data_as(dp), f.shape[0], n_obj, r.ctypes.data_as(dp),
                              out.ctypes.data, cap, _C.byref(cnt))
        if st == _lib.ERR_WORKSPACE and cnt.value > cap:   # retry with the reported count
            cap = int(cnt.value)
            continue
        _lib.check(st, "bo_hvi_boxes")
        return out[: cnt.value].copy()


def hypervolume_improvement_exact(ucb, front, reference_point, prior_mean, prior_variance, out=None):
    """Exact HVI of every candidate's UCB vector over `front`: acq = HV(front u {u}) - HV(front),
    u_k = prior_mean_k + sqrt(prior_variance_k) * ucb[k] (ucb: the reference's standardised
    per-objective UCB array, [n_obj, M], numpy or HIP tensor).  Returns acq ([M], a device
    tensor, or numpy for numpy `ucb`); written into `out` when given (in place)."""
    dev = _dev_of(out, ucb)
    u = _Arg(ucb, dev)
    n_obj, n = u.t.shape
    boxes = torch.as_tensor(hypervolume_boxes(front, reference_point), device=dev)
    acq = _Arg(out, dev, write=True) if out is not None else None
    dst = acq.t if acq is not None else torch.empty(n, dtype=F64, device=dev)
    pm = np.asarray(prior_mean, dtype=np.float64)[:n_obj]
    sc = np.sqrt(np.asarray(prior_variance, dtype=np.float64)[:n_obj])
    _lib.check(_lib.load().bo_hypervolume_improvement_exact(
        dst.data_ptr(), u.ptr, u.t.stride(0), n, n_obj, _host_vec(pm, n_obj), _host_vec(sc, n_obj),
        boxes.data_ptr() if boxes.numel() else None, boxes.shape[0], stream_handle(dev)),
        "bo_hypervolume_improvement_exact")
    if acq is not None:
        acq.finish()
        return out
    return dst if isinstance(ucb, torch.Tensor) else dst.cpu().numpy()


def hvi_select_indices(acquisition_values, ucb, y_vector, n_evaluations, reference_point, prior_mean,
                       prior_variance, cands, evaluated_points, batch_size, offset=0, return_record=False,
                       mask=None):
    """The exact-HVI acquisition AND its batch selection in one device pass (bo_hvi_select_topq,
    batch_size <= BO_MAX_TOPQ): acquisition_values (device, [count]) receives the HVI of the UCB
    vector of every candidate of the shard [offset, offset + count) over the Pareto front of
    y_vector[:n_evaluations]; returns the global indices of the shard's best batch_size candidates
    not equal to an evaluated point (select_next_batch's order) -- or, `return_record`, the device
    record block [2 batch_size] (values, bit-cast int64 indices) for the multi-rank exchange.
    `mask`: this shard's ExclusionMask (updated here with evaluated_points; only the new rows
    are added) -- the selection then runs bo_hvi_select_topq_masked."""
    if batch_size > _lib.MAX_TOPQ:
        raise ValueError(f"hvi_select_indices handles batch_size <= {_lib.MAX_TOPQ}")
    front = _front_of(y_vector, n_evaluations, reference_point)
    dev = _dev_of(acquisition_values, ucb)
    u = _Arg(ucb, dev)
    acq = _Arg(acquisition_values, dev, write=True)
    n_obj, n = u.t.shape
    boxes = torch.as_tensor(hypervolume_boxes(front, reference_point), device=dev)
    rec = torch.empty(2 * batch_size, dtype=F64, device=dev)
    lib = _lib.load()
    ws = Workspace.get(lib.bo_select_topq_workspace_size(n, batch_size), dev)
    shift = _host_vec(prior_mean, n_obj)
    scale = _host_vec(np.sqrt(np.asarray(prior_variance, dtype=np.float64)), n_obj)
    if mask is not None:
        _shard_mask(mask, cands, offset, n, dev, evaluated_points, "hvi_select_indices")
        _lib.check(lib.bo_hvi_select_topq_masked(acq.ptr, u.ptr, u.t.stride(0), n, n_obj, shift, scale,
                                                 boxes.data_ptr() if boxes.numel() else None, boxes.shape[0],
                                                 offset, mask.ptr, batch_size, rec.data_ptr(),
                                                 rec.data_ptr() + 8 * batch_size, ws.data_ptr(), ws.numel(),
                                                 stream_handle(dev)), "bo_hvi_select_topq_masked")
    else:
        ev = np.asarray(evaluated_points.cpu().numpy() if isinstance(evaluated_points, torch.Tensor)
                        else evaluated_points, dtype=np.float64).reshape(-1, cands.dim)
        ex = torch.as_tensor(np.ascontiguousarray(ev), device=dev)
        lo, sh = _grid_args(cands)
        carg = cands.cand_arg
        if cands.kind in ("i64", "f64"):            # explicit candidates: the shard's rows
            carg = cands.tensor[offset:].data_ptr()
        _lib.check(lib.bo_hvi_select_topq(acq.ptr, u.ptr, u.t.stride(0), n, n_obj, shift, scale,
                                          boxes.data_ptr() if boxes.numel() else None, boxes.shape[0],
                                          cands.kind_code, carg, lo, sh, cands.dim, offset,
                                          ex.data_ptr() if ex.numel() else None, ex.shape[0], batch_size,
                                          rec.data_ptr(), rec.data_ptr() + 8 * batch_size, ws.data_ptr(),
                                          ws.numel(), stream_handle(dev)), "bo_hvi_select_topq")
    acq.finish()
    return rec if return_record else _record_indices(rec, batch_size)


# ------------------------------------------------- expected hypervolume improvement (EHVI)
EHVI_FORMS = {"auto": 0, "direct": 1, "table": 2}


def ehvi_tables(boxes):
    """The table form's view of `boxes` (hypervolume_boxes' output, host [n_boxes, 2 n_obj]):
    (edges, box_idx) -- edges[k] the sorted unique finite bounds of objective k, box_idx int32
    [n_boxes, 2 n_obj] indices into them, len(edges[k]) standing for +inf (bo_ehvi_tables)."""
    b = np.ascontiguousarray(np.asarray(boxes, dtype=np.float64))
    n_obj = b.shape[1] // 2
    lib = _lib.load()
    ne = (_C.c_int32 * n_obj)()
    idx = np.empty((b.shape[0], 2 * n_obj), dtype=np.int32)
    cap = 64
    while True:
        flat = np.empty(cap, dtype=np.float64)
        st = lib.bo_ehvi_tables(b.ctypes.data, b.shape[0], n_obj, flat.ctypes.data, cap, ne, idx.ctypes.data)
        if st == _lib.ERR_WORKSPACE and sum(ne) > cap:      # retry with the reported counts
            cap = sum(ne)
            continue
        _lib.check(st, "bo_ehvi_tables")
        offs = np.concatenate([[0], np.cumsum(list(ne))])
        return [flat[offs[k]:offs[k + 1]].copy() for k in range(n_obj)], idx


class EhviTables:
    """What the EHVI scan reads besides mu / var, on the device: the boxes of the region `front`
    does not dominate above `reference_point` (direct form) and their edge tables (table form).
    Built once per front; `threads` is the table form's workgroup size, 0 when no table fits
    (`log_threads`: the same for the log-space scan, whose table holds 16 bytes per edge)."""

    def __init__(self, front, reference_point, device=None):
        self.dev = require_device(device)
        boxes = hypervolume_boxes(front, reference_point)
        self.n_obj = boxes.shape[1] // 2
        self.n_boxes = boxes.shape[0]
        edges, idx = ehvi_tables(boxes)
        self.n_edges = (_C.c_int32 * self.n_obj)(*[len(e) for e in edges])
        self.sum_edges = int(sum(self.n_edges))
        self.threads = int(_lib.load().bo_ehvi_table_threads(self.sum_edges))
        self.log_threads = int(_lib.load().bo_logehvi_table_threads(self.sum_edges))    # bo_log_ehvi's table
        self.boxes = torch.as_tensor(boxes, device=self.dev)
        self.edges = torch.as_tensor(np.concatenate(edges) if edges else np.zeros(0), device=self.dev)
        self.box_idx = torch.as_tensor(idx, device=self.dev)


def expected_hypervolume_improvement(mu, var, front, reference_point, out=None, form="auto", tables=None):
    """EHVI of every candidate over `front` above `reference_point` (maximisation; independent
    objectives Y_k ~ N(mu[k], |var[k]|), the predict's mu_objectives / variance_objectives in
    objective units, [n_obj, M], numpy or HIP tensors):
    acq = sum_b prod_k [psi_k(l_bk) - psi_k(u_bk)] over hypervolume_boxes' boxes,
    psi_k(a) = E[(Y_k - a)+] (bo_expected_hypervolume_improvement).  Not in the reference.
    `form`: "auto", "direct" or "table" (same bits; "table" raises where no table fits the LDS).
    `tables`: an EhviTables of the front, instead of `front` / `reference_point`.  Returns acq
    ([M], a device tensor, or numpy for numpy `mu`); written into `out` when given (in place)."""
    if form not in EHVI_FORMS:
        raise ValueError(f"unknown form {form!r} (expected 'auto', 'direct' or 'table')")
    dev = _dev_of(out, mu)
    m = _Arg(mu, dev)
    v = _Arg(var, dev)
    n_obj, n = m.t.shape
    if m.t.dim() != 2 or v.t.shape != m.t.shape:
        raise ValueError("mu / var must both be [n_obj, M]")
    tb = tables if tables is not None else EhviTables(front, reference_point, dev)
    if tb.n_obj != n_obj:
        raise ValueError(f"the front has {tb.n_obj} objectives, mu {n_obj}")
    acq = _Arg(out, dev, write=True) if out is not None else None
    dst = acq.t if acq is not None else torch.empty(n, dtype=F64, device=dev)
    if dst.numel() != n:
        raise ValueError(f"out holds {dst.numel()} values for {n} candidates")
    nb = tb.n_boxes
    _lib.check(_lib.load().bo_expected_hypervolume_improvement(
        dst.data_ptr(), m.ptr, v.ptr, n, n, n_obj,
        tb.boxes.data_ptr() if nb else None, nb, tb.edges.data_ptr() if nb else None, tb.n_edges,
        tb.box_idx.data_ptr() if nb else None, EHVI_FORMS[form], stream_handle(dev)),
        "bo_expected_hypervolume_improvement")
    if acq is not None:
        acq.finish()
        return out
    return dst if isinstance(mu, torch.Tensor) else dst.cpu().numpy()


def constrained_expected_hypervolume_improvement(mu, var, front, reference_point, constraint_bounds, out=None,
                                                 pof_out=None, form="auto", tables=None):
    """The feasibility-weighted EHVI of every candidate (bo_constrained_ehvi; include/bo_amd.h states
    the quantity, its limits and its rounding rule).  mu / var: [n_obj + n_con, M], the objective
    rows first (n_obj = len(reference_point), or tables.n_obj), numpy or HIP tensors.
    constraint_bounds: n_con pairs (lo, hi), either infinite on its own side.  `front`: the FEASIBLE
    evaluated points' objective vectors.  acq = EHVI(objective rows over `front`) * prod_j P_j,
    P_j = P(lo_j <= Y_j <= hi_j); `pof_out` ([M]) receives prod_j P_j.  `form` / `tables` as
    expected_hypervolume_improvement's (same bits).  No constraints: the plain EHVI's bits.
    Returns acq ([M], a device tensor, or numpy for numpy `mu`); written into `out` when given."""
    if form not in EHVI_FORMS:
        raise ValueError(f"unknown form {form!r} (expected 'auto', 'direct' or 'table')")
    bounds = check_constraint_bounds(constraint_bounds)
    n_con = bounds.shape[0]
    dev = _dev_of(out, mu)
    m = _Arg(mu, dev)
    v = _Arg(var, dev)
    if m.t.dim() != 2 or v.t.shape != m.t.shape or m.t.stride(1) != 1 or v.t.stride() != m.t.stride():
        raise ValueError("mu / var must both be [n_obj + n_con, M] with one row stride")
    n_out, n = m.t.shape
    tb = tables if tables is not None else EhviTables(front, reference_point, dev)
    n_obj = tb.n_obj
    if n_obj + n_con != n_out:
        raise ValueError(f"the front has {n_obj} objectives and there are {n_con} constraints, mu has {n_out} rows")
    acq = _Arg(out, dev, write=True) if out is not None else None
    dst = acq.t if acq is not None else torch.empty(n, dtype=F64, device=dev)
    if dst.numel() != n:
        raise ValueError(f"out holds {dst.numel()} values for {n} candidates")
    pof = _Arg(pof_out, dev, write=True) if pof_out is not None else None
    if pof is not None and pof.t.numel() != n:
        raise ValueError(f"pof_out holds {pof.t.numel()} values for {n} candidates")
    nb = tb.n_boxes
    _lib.check(_lib.load().bo_constrained_ehvi(
        dst.data_ptr(), pof.ptr if pof is not None else None, m.ptr, v.ptr, m.t.stride(0), n, n_obj, n_con,
        _host_vec(bounds[:, 0], n_con), _host_vec(bounds[:, 1], n_con),
        tb.boxes.data_ptr() if nb else None, nb, tb.edges.data_ptr() if nb else None, tb.n_edges,
        tb.box_idx.data_ptr() if nb else None, EHVI_FORMS[form], stream_handle(dev)), "bo_constrained_ehvi")
    if pof is not None:
        pof.finish()
    if acq is not None:
        acq.finish()
        return out
    return dst if isinstance(mu, torch.Tensor) else dst.cpu().numpy()


def update_expected_hypervolume_improvement(acquisition_values, mu_objectives, variance_objectives, y_vector,
                                            n_evaluations, reference_point, constraint_bounds=None):
    """The acquisition update of the loop (bayesian_optimization.py:195-199) as the EHVI: the front
    is the Pareto-efficient subset (device filter, pareto.py:12-45) of the evaluated objectives
    y_vector[:n_evaluations]; in place into `acquisition_values`.  With `constraint_bounds` (y_vector
    and mu / variance then carry the constraint outputs after the objectives): the constrained EHVI
    over the front of the feasible evaluated points."""
    if constraint_bounds is not None:
        constrained_expected_hypervolume_improvement(
            mu_objectives, variance_objectives,
            _front_of(y_vector, n_evaluations, reference_point, constraint_bounds), reference_point,
            constraint_bounds, out=acquisition_values)
        return
    expected_hypervolume_improvement(mu_objectives, variance_objectives,
                                     _front_of(y_vector, n_evaluations, reference_point), reference_point,
                                     out=acquisition_values)


def log_expected_hypervolume_improvement(mu, var, front, reference_point, constraint_bounds=None, out=None,
                                         logpof_out=None, form="auto", tables=None):
    """The natural logarithm of the EHVI -- with `constraint_bounds`, of the feasibility-weighted EHVI -- of
    every candidate (bo_log_ehvi; include/bo_amd.h states the quantity, its limits and its rounding rule):
    finite and correctly ordered where expected_hypervolume_improvement underflows to 0.0, -inf where the
    exact value is 0, NaN where any row holds NaN.  mu / var: [n_obj + n_con, M], the objective rows first
    (n_obj = len(reference_point), or tables.n_obj), numpy or HIP tensors; `front` with constraints: the
    FEASIBLE evaluated points' objective vectors.  `logpof_out` ([M]) receives sum_j ln P_j.  `form` /
    `tables` as expected_hypervolume_improvement's (same bits in both forms; the table holds 16 bytes per
    edge and thread, EhviTables.log_threads).  Returns the values ([M], a device tensor, or numpy for numpy
    `mu`); written into `out` when given (in place)."""
    if form not in EHVI_FORMS:
        raise ValueError(f"unknown form {form!r} (expected 'auto', 'direct' or 'table')")
    bounds = check_constraint_bounds(constraint_bounds)
    n_con = bounds.shape[0]
    dev = _dev_of(out, mu)
    m = _Arg(mu, dev)
    v = _Arg(var, dev)
    if m.t.dim() != 2 or v.t.shape != m.t.shape or m.t.stride(1) != 1 or v.t.stride() != m.t.stride():
        raise ValueError("mu / var must both be [n_obj + n_con, M] with one row stride")
    n_out, n = m.t.shape
    tb = tables if tables is not None else EhviTables(front, reference_point, dev)
    n_obj = tb.n_obj
    if n_obj + n_con != n_out:
        raise ValueError(f"the front has {n_obj} objectives and there are {n_con} constraints, mu has {n_out} rows")
    acq = _Arg(out, dev, write=True) if out is not None else None
    dst = acq.t if acq is not None else torch.empty(n, dtype=F64, device=dev)
    if dst.numel() != n:
        raise ValueError(f"out holds {dst.numel()} values for {n} candidates")
    lpo = _Arg(logpof_out, dev, write=True) if logpof_out is not None else None
    if lpo is not None and lpo.t.numel() != n:
        raise ValueError(f"logpof_out holds {lpo.t.numel()} values for {n} candidates")
    nb = tb.n_boxes
    if n > 0:                                              # an empty tensor has no address to pass
        _lib.check(_lib.load().bo_log_ehvi(
            dst.data_ptr(), lpo.ptr if lpo is not None else None, m.ptr, v.ptr, max(m.t.stride(0), n), n, n_obj, n_con,
            _host_vec(bounds[:, 0], n_con), _host_vec(bounds[:, 1], n_con),
            tb.boxes.data_ptr() if nb else None, nb, tb.edges.data_ptr() if nb else None, tb.n_edges,
            tb.box_idx.data_ptr() if nb else None, EHVI_FORMS[form], stream_handle(dev)), "bo_log_ehvi")
    if lpo is not None:
        lpo.finish()
    if acq is not None:
        acq.finish()
        return out
    return dst if isinstance(mu, torch.Tensor) else dst.cpu().numpy()


def update_log_expected_hypervolume_improvement(acquisition_values, mu_objectives, variance_objectives, y_vector,
                                                n_evaluations, reference_point, constraint_bounds=None):
    """update_expected_hypervolume_improvement with the log-space scan (acquisition "logehvi"): the same
    front (of the feasible rows with `constraint_bounds`), in place into `acquisition_values`."""
    log_expected_hypervolume_improvement(
        mu_objectives, variance_objectives, _front_of(y_vector, n_evaluations, reference_point, constraint_bounds),
        reference_point, constraint_bounds=constraint_bounds, out=acquisition_values)


def ehvi_select_indices(acquisition_values, mu_objectives, variance_objectives, y_vector, n_evaluations,
                        reference_point, cands, evaluated_points, batch_size, offset=0, return_record=False,
                        mask=None, constraint_bounds=None, log=False):
    """The EHVI acquisition and its batch selection over one shard, in two launches: the EHVI scan
    into acquisition_values (device, [count]: the candidates [offset, offset + count) of `cands`,
    over the Pareto front of y_vector[:n_evaluations]), then bo_select_topq_masked over the shard's
    ExclusionMask (`mask`, updated here with evaluated_points; without one a mask is built for the
    call).  batch_size <= BO_MAX_TOPQ.  Returns the global indices of the shard's best batch_size
    candidates not equal to an evaluated point (select_next_batch's order, NaN first) -- or,
    `return_record`, the device record block [2 batch_size] (values, bit-cast int64 indices) for
    the multi-rank exchange, as hvi_select_indices.  With `constraint_bounds` the scan is the
    constrained EHVI (constrained_expected_hypervolume_improvement) over the front of the feasible
    rows of y_vector; infeasible evaluated points stay excluded like any evaluated point.  `log`: the
    scan is log_expected_hypervolume_improvement (acquisition "logehvi"), the same selection over its
    values; a free candidate whose value is -inf is an ordinary, lowest, value of that order."""
    if batch_size > _lib.MAX_TOPQ:
        raise ValueError(f"ehvi_select_indices handles batch_size <= {_lib.MAX_TOPQ}")
    dev = _dev_of(acquisition_values, mu_objectives)
    acq = _Arg(acquisition_values, dev, write=True)
    n = acq.t.numel()
    mask = _shard_mask(mask, cands, offset, n, dev, evaluated_points, "ehvi_select_indices")
    if log:
        log_expected_hypervolume_improvement(
            mu_objectives, variance_objectives,
            _front_of(y_vector, n_evaluations, reference_point, constraint_bounds), reference_point,
            constraint_bounds=constraint_bounds, out=acq.t)
    elif constraint_bounds is not None:
        constrained_expected_hypervolume_improvement(
            mu_objectives, variance_objectives,
            _front_of(y_vector, n_evaluations, reference_point, constraint_bounds), reference_point,
            constraint_bounds, out=acq.t)
    else:
        expected_hypervolume_improvement(mu_objectives, variance_objectives,
                                         _front_of(y_vector, n_evaluations, reference_point), reference_point,
                                         out=acq.t)
    rec = torch.empty(2 * batch_size, dtype=F64, device=dev)
    lib = _lib.load()
    ws = Workspace.get(lib.bo_select_topq_workspace_size(n, batch_size), dev)
    _lib.check(lib.bo_select_topq_masked(acq.ptr, n, offset, mask.ptr, batch_size, rec.data_ptr(),
                                         rec.data_ptr() + 8 * batch_size, ws.data_ptr(), ws.numel(),
                                         stream_handle(dev)), "bo_select_topq_masked")
    acq.finish()
    return rec if return_record else _record_indices(rec, batch_size)


BATCH_STRATEGIES = ("top", "bucb", "ts")


def select_batch_bucb(std_mu_objectives, variance_objectives, x_train, kinv, cands, prior_variance,
                      length_scales, betas, evaluated_points, batch_size, offset=0, count=None, mask=None,
                      float_type=None, jitter=None, min_variance=None, return_variance=False,
                      return_details=False):
    """A batch whose later picks account for the earlier ones (GP-BUCB, Desautels, Krause &
    Burdick 2014; bo_select_batch_bucb).  NOT in the reference: select_next_batch
    (acquisition.py:116-144) takes the batch_size best values of one acquisition array, which on a
    smooth posterior are neighbours of one maximum.  Here pick t is the best candidate of the
    summed standardised UCB recomputed with the variance conditioned on picks 1..t-1 as
    hallucinated observations (the mean does not change); the first pick is select_next_batch's.

    std_mu_objectives / variance_objectives: the predict's outputs over the shard
    [offset, offset + count) of `cands` (device [n_obj, >= count], not modified); x_train [N, d] and
    kinv [n_obj, N, N] the fitted state the predict used.  `mask`: this shard's ExclusionMask,
    updated here with evaluated_points (only the new rows are added); without one a mask is built
    for the call.  jitter / min_variance default to KERNEL_JITTER / MIN_VARIANCE of `float_type`'s
    branch (config.precision_constants).  One device call, no host synchronisation between the
    picks.  Returns the global indices of the picks (fewer than batch_size when the shard runs out
    of candidates) -- with `return_variance`, also the conditioned variance (device
    [n_obj, count]); with `return_details`, a dict (top_idx, top_val, var, acq: device tensors)."""
    from .config import precision_constants
    if not 1 <= batch_size <= _lib.MAX_TOPQ:
        raise ValueError(f"select_batch_bucb handles 1 <= batch_size <= {_lib.MAX_TOPQ}")
    dev = _dev_of(std_mu_objectives, variance_objectives)
    smu = _Arg(std_mu_objectives, dev)
    var = _Arg(variance_objectives, dev)
    n_obj = smu.t.shape[0]
    count = int(cands.n - offset if count is None else count)
    if smu.t.dim() != 2 or var.t.shape != smu.t.shape or smu.t.shape[1] < count or smu.t.stride(1) != 1 \
            or var.t.stride() != smu.t.stride():
        raise ValueError("std_mu / variance must be [n_obj, >= count] with one row stride")
    x = torch.as_tensor(x_train, dtype=F64, device=dev).contiguous()
    kinv = torch.as_tensor(kinv, dtype=F64, device=dev).contiguous()
    n = x.shape[0]
    if not _fitted_ok(x, kinv, cands.dim, n_obj):
        raise ValueError("x_train must be [N, d] and kinv [n_obj, >=N, >=N]")
    kj, _, mv = precision_constants(float_type)
    mask = _shard_mask(mask, cands, offset, count, dev, evaluated_points, "select_batch_bucb")
    d = _lib.BucbDesc()
    d.n_obj, d.n_train, d.q = n_obj, n, batch_size
    d.x_train, d.kinv, d.ld_k = x.data_ptr(), kinv.data_ptr(), kinv.shape[-1]
    _set_cand_fields(d, cands, offset, count)
    for o in range(n_obj):
        d.prior_var[o] = float(prior_variance[o])
        d.length_scale[o] = float(length_scales[o])
        d.beta[o] = float(betas[o])
    d.jitter = float(kj if jitter is None else jitter)
    d.min_variance = float(mv if min_variance is None else min_variance)
    d.std_mu, d.var, d.ld = smu.ptr, var.ptr, smu.t.stride(0)
    d.mask = mask.ptr
    tv = torch.empty(batch_size, dtype=F64, device=dev)
    ti = torch.empty(batch_size, dtype=torch.int64, device=dev)
    d.top_val, d.top_idx = tv.data_ptr(), ti.data_ptr()
    var_out = acq_out = None
    if return_variance or return_details:
        var_out = torch.empty_like(var.t)
        d.var_out = var_out.data_ptr()
    if return_details:
        acq_out = torch.empty(count, dtype=F64, device=dev)
        d.acq_out = acq_out.data_ptr()
    lib = _lib.load()
    nbytes = lib.bo_select_batch_bucb_workspace_size(d)
    if nbytes == 0:
        raise _lib.BoNativeError(_lib.ERR_ARG, "bo_select_batch_bucb_workspace_size")
    ws = Workspace.get(nbytes, dev)
    _lib.check(lib.bo_select_batch_bucb(d, ws.data_ptr(), ws.numel(), stream_handle(dev)),
               "bo_select_batch_bucb")
    if return_details:
        return {"top_idx": ti, "top_val": tv, "var": var_out[:, :count], "acq": acq_out}
    idx = ti.cpu().numpy()
    idx = idx[idx >= 0].astype(np.int64)
    return (idx, var_out[:, :count]) if return_variance else idx


ALL_BATCH_STRATEGIES = BATCH_STRATEGIES + ("kb",)      # "kb": with acquisition="ehvi" only


class PinnedStaging:
    """Grow-only pinned host buffer, one per (device, stream), cached like Workspace: the staging
    block of select_batch_kb (bo_select_batch_kb hands it back on return, so the next call on
    the stream may rewrite it)."""

    _cache = {}

    @classmethod
    def get(cls, nbytes, device, stream=None):
        st = stream_handle(device) if stream is None else stream
        key = (device.type, device.index, int(st or 0))
        buf = cls._cache.get(key)
        if buf is None or buf.numel() < nbytes:
            size = max(int(nbytes), 0 if buf is None else buf.numel() + buf.numel() // 2, 4096)
            buf = torch.empty(size, dtype=torch.uint8, pin_memory=True)
            cls._cache[key] = buf
        return buf


_KB_BOX_CAPACITY = {}          # n_obj -> the box capacity the last call needed


def select_batch_kb(mu_objectives, variance_objectives, x_train, kinv, cands, prior_variance, length_scales,
                    y_vector, n_evaluations, reference_point, evaluated_points, batch_size, offset=0, count=None,
                    mask=None, float_type=None, jitter=None, min_variance=None, form="auto", acq_out=None,
                    return_details=False, box_capacity=None):
    """A batch for the EHVI whose later picks account for the earlier ones (Kriging believer,
    Ginsbourger, Le Riche & Carraro 2010; bo_select_batch_kb, include/bo_amd.h states the
    definition).  NOT in the reference.  Pick t is the best candidate of the EHVI of
    (mu, var conditioned on picks 1..t-1) over the Pareto front of y_vector[:n_evaluations]
    extended by the posterior means at those picks (the believed observations; the mean does not
    move); the first pick is ehvi_select_indices' top-1.

    mu_objectives / variance_objectives: the predict's outputs in objective units over the shard
    [offset, offset + count) of `cands` (device [n_obj, >= count], not modified); x_train [N, d]
    and kinv [n_obj, N, N] the fitted state the predict used.  `mask`: this shard's ExclusionMask,
    updated here with evaluated_points; without one a mask is built for the call.  jitter /
    min_variance default to KERNEL_JITTER / MIN_VARIANCE of `float_type`'s branch.  `form`: "auto",
    "direct" or "table" as expected_hypervolume_improvement's (same bits).  `acq_out` (device
    [count]) receives the first pick's acquisition, the plain EHVI array.  The box decomposition
    runs on the host between the picks, so the call synchronises with the stream once per pick
    (pinned staging and the device workspace are cached); when a pick's boxes exceed the device
    buffers (`box_capacity`, default: what the last call needed, at least 1024) the call is
    repeated from the start with the reported count rounded up -- the picks are deterministic.
    Returns the global indices of the picks (fewer than batch_size when the shard runs out of
    candidates); with `return_details`, a dict (top_idx, top_val, var, acq_first, acq_last,
    believed: device tensors; n_boxes_max: int)."""
    from .config import precision_constants
    if not 1 <= batch_size <= _lib.MAX_TOPQ:
        raise ValueError(f"select_batch_kb handles 1 <= batch_size <= {_lib.MAX_TOPQ}")
    if form not in EHVI_FORMS:
        raise ValueError(f"unknown form {form!r} (expected 'auto', 'direct' or 'table')")
    dev = _dev_of(mu_objectives, variance_objectives)
    mu = _Arg(mu_objectives, dev)
    var = _Arg(variance_objectives, dev)
    n_obj = mu.t.shape[0]
    if n_obj > 4:
        raise ValueError(f"select_batch_kb supports at most 4 objectives (got {n_obj})")
    count = int(cands.n - offset if count is None else count)
    if mu.t.dim() != 2 or var.t.shape != mu.t.shape or mu.t.shape[1] < count or mu.t.stride(1) != 1 \
            or var.t.stride() != mu.t.stride():
        raise ValueError("mu / variance must be [n_obj, >= count] with one row stride")
    x = torch.as_tensor(x_train, dtype=F64, device=dev).contiguous()
    kinv = torch.as_tensor(kinv, dtype=F64, device=dev).contiguous()
    n = x.shape[0]
    if not _fitted_ok(x, kinv, cands.dim, n_obj):
        raise ValueError("x_train must be [N, d] and kinv [n_obj, >=N, >=N]")
    ref = np.asarray(reference_point, dtype=np.float64).ravel()
    if ref.size != n_obj:
        raise ValueError(f"the reference point has {ref.size} objectives, mu {n_obj}")
    front = np.ascontiguousarray(np.asarray(_front_of(y_vector, n_evaluations, ref), dtype=np.float64)
                                 .reshape(-1, n_obj))
    kj, _, mv = precision_constants(float_type)
    mask = _shard_mask(mask, cands, offset, count, dev, evaluated_points, "select_batch_kb")
    d = _lib.KbDesc()
    d.n_obj, d.n_train, d.q = n_obj, n, batch_size
    d.x_train, d.kinv, d.ld_k = x.data_ptr(), kinv.data_ptr(), kinv.shape[-1]
    _set_cand_fields(d, cands, offset, count)
    for o in range(n_obj):
        d.prior_var[o] = float(prior_variance[o])
        d.length_scale[o] = float(length_scales[o])
        d.ref_point[o] = float(ref[o])
    d.jitter = float(kj if jitter is None else jitter)
    d.min_variance = float(mv if min_variance is None else min_variance)
    d.mu, d.var, d.ld = mu.ptr, var.ptr, mu.t.stride(0)
    d.mask = mask.ptr
    d.front, d.n_front = (front.ctypes.data if front.shape[0] else None), front.shape[0]
    d.form = EHVI_FORMS[form]
    tv = torch.empty(batch_size, dtype=F64, device=dev)
    ti = torch.empty(batch_size, dtype=torch.int64, device=dev)
    believed = torch.empty((batch_size, n_obj), dtype=F64, device=dev)
    d.top_val, d.top_idx, d.believed = tv.data_ptr(), ti.data_ptr(), believed.data_ptr()
    var_out = acq_last = None
    acq_first = _Arg(acq_out, dev, write=True) if acq_out is not None else None
    if acq_first is not None and acq_first.t.numel() != count:
        raise ValueError(f"acq_out holds {acq_first.t.numel()} values for {count} candidates")
    first = acq_first.t if acq_first is not None else None
    if return_details:
        var_out = torch.empty_like(var.t)
        d.var_out = var_out.data_ptr()
        acq_last = torch.empty(count, dtype=F64, device=dev)
        d.acq_last = acq_last.data_ptr()
        if first is None:
            first = torch.empty(count, dtype=F64, device=dev)
    if first is not None:
        d.acq_first = first.data_ptr()
    met = C_i64(0)
    d.n_boxes_max = _C.pointer(met)
    lib = _lib.load()
    cap = int(box_capacity) if box_capacity is not None else max(1024, _KB_BOX_CAPACITY.get(n_obj, 0))
    for attempt in range(4):
        d.box_capacity = cap
        nbytes = lib.bo_select_batch_kb_workspace_size(d)
        hbytes = lib.bo_select_batch_kb_host_workspace_size(d)
        if nbytes == 0 or hbytes == 0:
            raise _lib.BoNativeError(_lib.ERR_ARG, "bo_select_batch_kb_workspace_size")
        ws = Workspace.get(nbytes, dev)
        hws = PinnedStaging.get(hbytes, dev)
        d.host_ws, d.host_ws_bytes = hws.data_ptr(), hws.numel()
        st = lib.bo_select_batch_kb(d, ws.data_ptr(), ws.numel(), stream_handle(dev))
        if st == _lib.ERR_WORKSPACE and met.value > cap and attempt < 3:
            cap = (2 * int(met.value) + 255) // 256 * 256   # the count that did not fit, rounded up
            continue
        _lib.check(st, "bo_select_batch_kb")
        break
    if box_capacity is None:
        _KB_BOX_CAPACITY[n_obj] = cap
    if acq_first is not None:
        acq_first.finish()
    if return_details:
        return {"top_idx": ti, "top_val": tv, "var": var_out[:, :count], "acq_first": first, "acq_last": acq_last,
                "believed": believed, "n_boxes_max": int(met.value)}
    idx = ti.cpu().numpy()
    return idx[idx >= 0].astype(np.int64)


def update_hypervolume_improvement_exact(acquisition_values, ucb, y_vector, n_evaluations,
                                         reference_point, prior_mean, prior_variance):
    """The acquisition update of the loop (bayesian_optimization.py:195-199) as an exact HVI:
    the front is the Pareto-efficient subset (device filter, pareto.py:12-45) of the evaluated
    objectives y_vector[:n_evaluations]; in place into `acquisition_values`."""
    hypervolume_improvement_exact(ucb, _front_of(y_vector, n_evaluations, reference_point), reference_point, prior_mean, prior_variance,
                                  out=acquisition_values)


# ------------------------------------------------- Thompson-sampling batches (pathwise draws)
def thompson_draws(rng, n_obj, dim, n_train, n_samples, n_features):
    """The random numbers of bo_sample_paths from a numpy.random.Generator `rng` (never numpy's
    global RNG: config.py seeds that one and the LHS design depends on its draw order):
    (Z [n_obj, D, dim] standard normals, B [n_obj, D] uniform on [0, 2 pi), Theta [S, n_obj, D] and
    E [S, n_obj, N] standard normals), float64, in this order of draws."""
    if not isinstance(rng, np.random.Generator):
        raise TypeError("thompson_draws needs a numpy.random.Generator (numpy.random.default_rng(seed))")
    z = rng.standard_normal((n_obj, n_features, dim))
    b = rng.uniform(0.0, 2.0 * np.pi, (n_obj, n_features))
    theta = rng.standard_normal((n_samples, n_obj, n_features))
    eps = rng.standard_normal((n_samples, n_obj, n_train))
    return z, b, theta, eps


def sample_paths(x_train, y_train, kinv, cands, prior_mean, prior_variance, length_scales, draws, offset=0,
                 count=None, float_type=None, jitter=None, ld=None, return_weights=False, device=None):
    """Posterior function draws over the shard [offset, offset + count) of `cands` by pathwise
    conditioning over random Fourier features (bo_sample_paths; include/bo_amd.h states the
    definition).  x_train [N, d], y_train [N, n_obj], kinv [n_obj, >= N, >= N]: the fitted state
    the predict uses; draws = (Z, B, Theta, E) as thompson_draws returns them (numpy or device).
    jitter defaults to KERNEL_JITTER of `float_type`'s branch.  Returns the device tensor
    [S, n_obj, count] of the standardised draws (f - prior_mean) / sqrt(prior_variance) (a view of
    [S, n_obj, ld] when `ld` is given) -- with `return_weights`, also the weights v [S, n_obj, N]
    that were used.  Deterministic: the same arguments give the same bits."""
    from .config import precision_constants
    dev = require_device(device) if device is not None else _dev_of(kinv, x_train)
    x = torch.as_tensor(x_train, dtype=F64, device=dev).contiguous()
    y = torch.as_tensor(y_train, dtype=F64, device=dev)
    kinv = torch.as_tensor(kinv, dtype=F64, device=dev).contiguous()
    n, n_obj = x.shape[0], kinv.shape[0]
    if y.dim() != 2 or y.stride(1) != 1:
        y = y.contiguous()
    z, b, theta, eps = (torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64) if isinstance(a, np.ndarray) else a,
                                        dtype=F64, device=dev).contiguous() for a in draws)
    if not _fitted_ok(x, kinv, cands.dim, n_obj) or y.shape[0] < n or y.shape[1] < n_obj:
        raise ValueError("x_train must be [N, d], y_train [N, n_obj] and kinv [n_obj, >=N, >=N]")
    if theta.dim() != 3 or z.dim() != 3:
        raise ValueError("draws must be (Z [n_obj, D, d], B [n_obj, D], Theta [S, n_obj, D], E [S, n_obj, N])")
    n_samples, n_feat = theta.shape[0], theta.shape[2]
    if tuple(z.shape) != (n_obj, n_feat, cands.dim) or tuple(b.shape) != (n_obj, n_feat) \
            or theta.shape[1] != n_obj or tuple(eps.shape) != (n_samples, n_obj, n):
        raise ValueError("draws must be (Z [n_obj, D, d], B [n_obj, D], Theta [S, n_obj, D], E [S, n_obj, N])")
    if not 1 <= n_samples <= _lib.MAX_TOPQ:
        raise ValueError(f"sample_paths handles 1 <= n_samples <= {_lib.MAX_TOPQ}")
    count = int(cands.n - offset if count is None else count)
    ld = count if ld is None else int(ld)
    d = _lib.TsDesc()
    d.n_obj, d.n_train = n_obj, n
    d.x_train, d.y, d.ld_y = x.data_ptr(), y.data_ptr(), y.stride(0)
    d.kinv, d.ld_k = kinv.data_ptr(), kinv.shape[-1]
    d.n_samples, d.n_features = n_samples, n_feat
    _set_cand_fields(d, cands, offset, count)
    for o in range(n_obj):
        d.prior_mean[o] = float(prior_mean[o])
        d.prior_var[o] = float(prior_variance[o])
        d.length_scale[o] = float(length_scales[o])
    d.jitter = float(precision_constants(float_type)[0] if jitter is None else jitter)
    d.z, d.phase, d.theta, d.eps = z.data_ptr(), b.data_ptr(), theta.data_ptr(), eps.data_ptr()
    paths = torch.empty((n_samples, n_obj, ld), dtype=F64, device=dev)
    d.paths, d.ld = paths.data_ptr(), ld
    wts = None
    if return_weights:
        wts = torch.empty((n_samples, n_obj, n), dtype=F64, device=dev)
        d.weights_out = wts.data_ptr()
    lib = _lib.load()
    nbytes = lib.bo_sample_paths_workspace_size(d)
    if nbytes == 0:
        raise _lib.BoNativeError(_lib.ERR_ARG, "bo_sample_paths_workspace_size")
    ws = Workspace.get(nbytes, dev)
    _lib.check(lib.bo_sample_paths(d, ws.data_ptr(), ws.numel(), stream_handle(dev)), "bo_sample_paths")
    out = paths[:, :, :count]
    return (out, wts) if return_weights else out


def resolve_ts_picks(lists):
    """Pick s = the first index of lists[s] (draw s's candidates, best first; negative = empty) that
    no earlier draw picked; -1 when none is left.  int64 [len(lists)]."""
    picks, taken = [], set()
    for idx in lists:
        p = -1
        for i in idx:
            i = int(i)
            if i >= 0 and i not in taken:
                p = i
                break
        if p >= 0:
            taken.add(p)
        picks.append(p)
    return np.asarray(picks, dtype=np.int64)


def select_batch_ts(x_train, y_train, kinv, cands, prior_mean, prior_variance, length_scales, draws,
                    evaluated_points, batch_size, acquisition="sum_ucb", y_evaluated=None, reference_point=None,
                    offset=0, count=None, mask=None, float_type=None, jitter=None, group=None,
                    return_details=False):
    """A Thompson-sampling batch: pick s is the best candidate of posterior draw s (sample_paths)
    under the acquisition -- "sum_ucb": the sum over the objectives of the standardised draw, the
    reference's scalarisation (acquisition.py:89-108) with the UCB replaced by the draw; "hvi": the
    exact hypervolume improvement of the drawn objective vector over the Pareto front of
    `y_evaluated` above `reference_point` (the TSEMO criterion) -- among the candidates that are
    neither evaluated nor picked by an earlier draw (select_next_batch's order).  NOT in the
    reference.  Draw s runs the existing masked selection with top-(s + 1), which always holds a
    candidate no earlier draw took; every record goes into one device block, read back once, and
    the picks are resolved in draw order on the host.  With collectives on, each draw's records are
    exchanged (exchange_topq_rec) and resolved on the merged lists: every rank scores the same draws
    (the caller hands every rank the same `draws`), so the picks are identical on every rank.
    Returns the global indices of the picks (fewer than batch_size when the candidates run out);
    `return_details`: a dict (picks with -1 markers [batch_size], paths, and per draw the record's
    indices `lists` and values `vals`)."""
    if acquisition not in ("sum_ucb", "hvi"):
        raise ValueError(f"select_batch_ts: acquisition {acquisition!r} has no sampled form "
                         "(expected 'sum_ucb' or 'hvi')")
    if not 1 <= batch_size <= _lib.MAX_TOPQ:
        raise ValueError(f"select_batch_ts handles 1 <= batch_size <= {_lib.MAX_TOPQ}")
    if np.shape(draws[2])[0] != batch_size:
        raise ValueError("select_batch_ts: draws must hold batch_size samples")
    count = int(cands.n - offset if count is None else count)
    paths = sample_paths(x_train, y_train, kinv, cands, prior_mean, prior_variance, length_scales, draws,
                         offset=offset, count=count, float_type=float_type, jitter=jitter)
    dev = paths.device
    n_obj = paths.shape[1]
    mask = _shard_mask(mask, cands, offset, count, dev, evaluated_points, "select_batch_ts")
    lib = _lib.load()
    st = stream_handle(dev)
    ws = Workspace.get(lib.bo_select_topq_workspace_size(count, batch_size), dev)
    acq = torch.empty(count, dtype=F64, device=dev)
    # draw s's record: s + 1 values, then s + 1 bit-cast int64 indices, at doubles [s (s + 1), ...)
    rec = torch.empty(batch_size * (batch_size + 1), dtype=F64, device=dev)
    if acquisition == "hvi":
        yv = np.asarray(y_evaluated, dtype=np.float64)
        front = _front_of(yv, len(yv), reference_point)
        boxes = torch.as_tensor(hypervolume_boxes(front, reference_point), device=dev)
        shift = _host_vec(prior_mean, n_obj)
        scale = _host_vec(np.sqrt(np.asarray(prior_variance, dtype=np.float64)), n_obj)
    for s in range(batch_size):
        q = s + 1
        tv = rec.data_ptr() + 8 * s * (s + 1)
        ti = tv + 8 * q
        p = paths[s]
        if acquisition == "sum_ucb":
            _lib.check(lib.bo_update_hypervolume_improvement(acq.data_ptr(), p.data_ptr(), n_obj, count, st),
                       "bo_update_hypervolume_improvement")
            _lib.check(lib.bo_select_topq_masked(acq.data_ptr(), count, offset, mask.ptr, q, tv, ti,
                                                 ws.data_ptr(), ws.numel(), st), "bo_select_topq_masked")
        else:
            _lib.check(lib.bo_hvi_select_topq_masked(acq.data_ptr(), p.data_ptr(), p.stride(0), count, n_obj,
                                                     shift, scale, boxes.data_ptr() if boxes.numel() else None,
                                                     boxes.shape[0], offset, mask.ptr, q, tv, ti, ws.data_ptr(),
                                                     ws.numel(), st), "bo_hvi_select_topq_masked")
    from .distributed import collectives_on, exchange_topq_rec
    lists, vals = [], []
    if collectives_on(group):
        for s in range(batch_size):
            q = s + 1
            v, i = exchange_topq_rec(rec[s * q: s * q + 2 * q], q, group)
            vals.append(np.asarray(v, dtype=np.float64))
            lists.append(np.asarray(i, dtype=np.int64))
    else:
        host = rec.cpu().numpy()                     # the one read-back
        for s in range(batch_size):
            q = s + 1
            vals.append(host[s * q: s * q + q].copy())
            lists.append(host[s * q + q: s * q + 2 * q].view(np.int64).copy())
    picks = resolve_ts_picks(lists)
    if return_details:
        return {"picks": picks, "paths": paths, "lists": lists, "vals": vals}
    return picks[picks >= 0]


# ------------------------------------------------- max-value entropy search (MESMO)
def path_maxima(paths, prior_mean, prior_variance, group=None):
    """The per-draw maxima of posterior draws in objective units (bo_path_maxima):
    ystar[s, k] = fl(prior_mean[k] + sqrt(prior_variance[k]) * max_c paths[s, k, c]), one rounding, NaN
    entries ignored (an all-NaN or empty row gives NaN).  paths: sample_paths' device tensor
    [S, n_obj, count] (a view with a larger row stride is taken as it is).  With collectives on, the
    ranks' maxima are combined by one all_reduce(MAX) -- the max is exact and the map monotone, so
    every rank then holds the bits of the unsharded call; the collective's tensor is on the device
    for RCCL and a host copy for gloo.  Returns a device tensor [S, n_obj].  NOT in the reference."""
    if not isinstance(paths, torch.Tensor) or paths.device.type != "cuda" or paths.dtype != F64 or paths.dim() != 3:
        raise ValueError("paths must be a float64 HIP tensor [S, n_obj, count]")
    n_s, n_obj, count = paths.shape
    if not 1 <= n_s <= _lib.MAX_TOPQ or not 1 <= n_obj <= _lib.MAX_OBJ:
        raise ValueError(f"path_maxima handles 1 <= S <= {_lib.MAX_TOPQ} and 1 <= n_obj <= {_lib.MAX_OBJ}")
    # the row stride of the [S n_obj][ld] layout the paths are a view of (a dimension of size 1 has none)
    ld = paths.stride(1) if n_obj > 1 else (paths.stride(0) if n_s > 1 else count)
    if (count > 1 and paths.stride(2) != 1) or (n_s > 1 and paths.stride(0) != n_obj * ld) or ld < count:
        paths = paths.contiguous()
        ld = count
    dev = paths.device
    lib = _lib.load()
    ystar = torch.empty((n_s, n_obj), dtype=F64, device=dev)
    ws = Workspace.get(lib.bo_path_maxima_workspace_size(count, n_s * n_obj), dev)
    scale = np.sqrt(np.asarray(prior_variance, dtype=np.float64))
    _lib.check(lib.bo_path_maxima(ystar.data_ptr(), paths.data_ptr(), ld, count, n_s, n_obj,
                                  _host_vec(prior_mean, n_obj), _host_vec(scale, n_obj), ws.data_ptr(), ws.numel(),
                                  stream_handle(dev)), "bo_path_maxima")
    from .distributed import collectives_on
    if collectives_on(group):
        import torch.distributed as dist
        if dist.get_backend(group) == "nccl":
            dist.all_reduce(ystar, op=dist.ReduceOp.MAX, group=group)
        else:                                       # gloo: the collective on a host copy
            h = ystar.cpu()
            dist.all_reduce(h, op=dist.ReduceOp.MAX, group=group)
            ystar.copy_(h)
    return ystar


def max_value_entropy(mu, var, ystar, out=None):
    """The max-value entropy search acquisition of every candidate (bo_max_value_entropy;
    include/bo_amd.h states the quantity, its limits and its rounding rule):
    acq = (1/S) sum_s sum_k g((ystar[s, k] - mu[k]) / sqrt(|var[k]|)),
    g(x) = x phi(x) / (2 Phi(x)) - ln Phi(x).  mu / var: the predict's mu_objectives /
    variance_objectives in objective units, [n_obj, M] with 1 <= n_obj <= 8, numpy or HIP tensors;
    ystar: [S, n_obj] sampled maxima (path_maxima), 1 <= S <= BO_MAX_TOPQ.  NOT in the reference.
    Returns acq ([M], a device tensor, or numpy for numpy `mu`); written into `out` when given."""
    dev = _dev_of(out, mu, ystar)
    m = _Arg(mu, dev)
    v = _Arg(var, dev)
    if m.t.dim() != 2 or v.t.shape != m.t.shape:
        raise ValueError("mu / var must both be [n_obj, M]")
    n_obj, n = m.t.shape
    ys = _Arg(ystar, dev)
    if ys.t.dim() != 2 or ys.t.shape[1] != n_obj:
        raise ValueError(f"ystar must be [S, n_obj] with n_obj = {n_obj}")
    n_s = ys.t.shape[0]
    if not 1 <= n_s <= _lib.MAX_TOPQ or not 1 <= n_obj <= _lib.MAX_OBJ:
        raise ValueError(f"max_value_entropy handles 1 <= S <= {_lib.MAX_TOPQ} and 1 <= n_obj <= {_lib.MAX_OBJ}")
    acq = _Arg(out, dev, write=True) if out is not None else None
    dst = acq.t if acq is not None else torch.empty(n, dtype=F64, device=dev)
    if dst.numel() != n:
        raise ValueError(f"out holds {dst.numel()} values for {n} candidates")
    _lib.check(_lib.load().bo_max_value_entropy(dst.data_ptr(), m.ptr, v.ptr, n, n, n_obj, ys.ptr, n_s,
                                                stream_handle(dev)), "bo_max_value_entropy")
    if acq is not None:
        acq.finish()
        return out
    return dst if isinstance(mu, torch.Tensor) else dst.cpu().numpy()


def update_max_value_entropy(acquisition_values, mu_objectives, variance_objectives, ystar):
    """The acquisition update of the loop (bayesian_optimization.py:195-199) as the max-value entropy
    search acquisition over the sampled maxima `ystar` ([S, n_obj], path_maxima); in place into
    `acquisition_values`."""
    max_value_entropy(mu_objectives, variance_objectives, ystar, out=acquisition_values)


MES_BATCH_STRATEGIES = ("top", "gibbon")               # the batches of acquisition="mes"


def select_batch_gibbon(base, variance_objectives, x_train, kinv, cands, prior_variance, length_scales,
                        evaluated_points, batch_size, offset=0, count=None, mask=None, float_type=None,
                        jitter=None, min_variance=None, return_variance=False, return_details=False):
    """A batch for an information criterion whose later picks account for the earlier ones (GIBBON's
    greedy batch bound, Moss, Leslie, Gonzalez & Rayson 2021; bo_select_batch_gibbon,
    include/bo_amd.h states the definition).  NOT in the reference.  The first pick is the masked
    top-1 of `base`; pick t > 1 is the best candidate of
    base + 0.5 sum_o log(var_o^(t-1) / var_o^0), where var^(t-1) is the variance conditioned on picks
    1..t-1 as hallucinated observations (select_batch_bucb's update) and var^0 the given one: the
    greedy increment of half the log-determinant of the batch's predictive correlation matrix.

    base: the single-point acquisition over the shard [offset, offset + count) of `cands` (device
    [count]; in the loop the max-value entropy array -- any array will do); variance_objectives:
    the predict's output over that shard (device [n_obj, >= count]); neither is modified.  x_train
    [N, d] and kinv [n_obj, N, N]: the fitted state the predict used.  `mask`: this shard's
    ExclusionMask, updated here with evaluated_points; without one a mask is built for the call.
    jitter / min_variance default to KERNEL_JITTER / MIN_VARIANCE of `float_type`'s branch.  One
    device call, no host synchronisation between the picks.  Returns the global indices of the
    picks (fewer than batch_size when the shard runs out of candidates) -- with `return_variance`,
    also the conditioned variance (device [n_obj, count]); with `return_details`, a dict (top_idx,
    top_val, var, acq_last: device tensors; acq_last is the array the last pick was taken from)."""
    from .config import precision_constants
    if not 1 <= batch_size <= _lib.MAX_TOPQ:
        raise ValueError(f"select_batch_gibbon handles 1 <= batch_size <= {_lib.MAX_TOPQ}")
    dev = _dev_of(base, variance_objectives)
    b = _Arg(base, dev)
    var = _Arg(variance_objectives, dev)
    if var.t.dim() != 2 or not 1 <= var.t.shape[0] <= _lib.MAX_OBJ:
        raise ValueError(f"variance must be [n_obj, >= count] with 1 <= n_obj <= {_lib.MAX_OBJ}")
    n_obj = var.t.shape[0]
    count = int(cands.n - offset if count is None else count)
    if var.t.shape[1] < count:
        raise ValueError(f"variance must be [n_obj, >= count] (count = {count})")
    if b.t.dim() != 1 or b.t.numel() != count:
        raise ValueError(f"base must hold one value for each of the {count} candidates")
    x = torch.as_tensor(x_train, dtype=F64, device=dev).contiguous()
    kinv = torch.as_tensor(kinv, dtype=F64, device=dev).contiguous()
    n = x.shape[0]
    if not _fitted_ok(x, kinv, cands.dim, n_obj):
        raise ValueError("x_train must be [N, d] and kinv [n_obj, >=N, >=N]")
    kj, _, mv = precision_constants(float_type)
    mask = _shard_mask(mask, cands, offset, count, dev, evaluated_points, "select_batch_gibbon")
    d = _lib.GibbonDesc()
    d.n_obj, d.n_train, d.q = n_obj, n, batch_size
    d.x_train, d.kinv, d.ld_k = x.data_ptr(), kinv.data_ptr(), kinv.shape[-1]
    _set_cand_fields(d, cands, offset, count)
    for o in range(n_obj):
        d.prior_var[o] = float(prior_variance[o])
        d.length_scale[o] = float(length_scales[o])
    d.jitter = float(kj if jitter is None else jitter)
    d.min_variance = float(mv if min_variance is None else min_variance)
    d.base, d.var = b.ptr, var.ptr
    d.ld = var.t.shape[1]                              # _Arg: contiguous
    d.mask = mask.ptr
    tv = torch.empty(batch_size, dtype=F64, device=dev)
    ti = torch.empty(batch_size, dtype=torch.int64, device=dev)
    d.top_val, d.top_idx = tv.data_ptr(), ti.data_ptr()
    var_out = acq_last = None
    if return_variance or return_details:
        var_out = torch.empty((n_obj, d.ld), dtype=F64, device=dev)
        d.var_out = var_out.data_ptr()
    if return_details:
        acq_last = torch.empty(count, dtype=F64, device=dev)
        d.acq_last = acq_last.data_ptr()
    lib = _lib.load()
    nbytes = lib.bo_select_batch_gibbon_workspace_size(d)
    if nbytes == 0:
        raise _lib.BoNativeError(_lib.ERR_ARG, "bo_select_batch_gibbon_workspace_size")
    ws = Workspace.get(nbytes, dev)
    _lib.check(lib.bo_select_batch_gibbon(d, ws.data_ptr(), ws.numel(), stream_handle(dev)),
               "bo_select_batch_gibbon")
    if return_details:
        return {"top_idx": ti, "top_val": tv, "var": var_out[:, :count], "acq_last": acq_last}
    idx = ti.cpu().numpy()
    idx = idx[idx >= 0].astype(np.int64)
    return (idx, var_out[:, :count]) if return_variance else idx


def mes_select_indices(acquisition_values, mu_objectives, variance_objectives, x_train, y_train, kinv, cands,
                       prior_mean, prior_variance, length_scales, draws, evaluated_points, batch_size, offset=0,
                       return_record=False, mask=None, float_type=None, jitter=None, group=None, select=True,
                       batch_strategy="top"):
    """The max-value entropy search acquisition and its batch selection over one shard, shaped like
    ehvi_select_indices: the posterior draws over the shard (sample_paths with `draws`, as
    thompson_draws returns them -- every rank the same), their maxima (path_maxima: over ALL
    candidates, the ranks' shards combined by one all_reduce(MAX) when collectives are on), the scan
    into acquisition_values (device, [count]: the candidates [offset, offset + count) of `cands`,
    from the predict's mu_objectives / variance_objectives over that shard), then
    bo_select_topq_masked over the shard's ExclusionMask (`mask`, updated here with
    evaluated_points; without one a mask is built for the call).  batch_size <= BO_MAX_TOPQ.
    Returns the global indices of the shard's best batch_size candidates not equal to an evaluated
    point (select_next_batch's order, NaN first) -- or, `return_record`, the device record block
    [2 batch_size] for the multi-rank exchange.  `select` False: the scan only (returns None).
    `batch_strategy` "gibbon" (one rank, so no record block): the scan as above, then
    select_batch_gibbon on it -- every pick after the first is penalised by half the log-ratio of
    the variance conditioned on the earlier picks to the unconditioned one (jitter as the draws',
    the floor of `float_type`'s branch); returns the global indices of the picks."""
    if batch_strategy not in MES_BATCH_STRATEGIES:
        raise ValueError(f"unknown batch_strategy {batch_strategy!r} for the max-value entropy "
                         f"(expected one of {MES_BATCH_STRATEGIES})")
    if batch_strategy == "gibbon" and (return_record or not select):
        raise ValueError("batch_strategy='gibbon' runs on one rank and returns its picks: it has no record block "
                         "and no scan-only form")
    if select and batch_size > _lib.MAX_TOPQ:
        raise ValueError(f"mes_select_indices handles batch_size <= {_lib.MAX_TOPQ}")
    dev = _dev_of(acquisition_values, mu_objectives)
    acq = _Arg(acquisition_values, dev, write=True)
    n = acq.t.numel()
    paths = sample_paths(x_train, y_train, kinv, cands, prior_mean, prior_variance, length_scales, draws,
                         offset=offset, count=n, float_type=float_type, jitter=jitter, device=dev)
    ystar = path_maxima(paths, prior_mean, prior_variance, group=group)
    max_value_entropy(mu_objectives, variance_objectives, ystar, out=acq.t)
    if not select:
        acq.finish()
        return None
    mask = _shard_mask(mask, cands, offset, n, dev, evaluated_points, "mes_select_indices")
    if batch_strategy == "gibbon":
        idx = select_batch_gibbon(acq.t, variance_objectives, x_train, kinv, cands, prior_variance, length_scales,
                                  evaluated_points, batch_size, offset=offset, count=n, mask=mask,
                                  float_type=float_type, jitter=jitter)
        acq.finish()
        return idx
    rec = torch.empty(2 * batch_size, dtype=F64, device=dev)
    lib = _lib.load()
    ws = Workspace.get(lib.bo_select_topq_workspace_size(n, batch_size), dev)
    _lib.check(lib.bo_select_topq_masked(acq.ptr, n, offset, mask.ptr, batch_size, rec.data_ptr(),
                                         rec.data_ptr() + 8 * batch_size, ws.data_ptr(), ws.numel(),
                                         stream_handle(dev)), "bo_select_topq_masked")
    acq.finish()
    return rec if return_record else _record_indices(rec, batch_size)

"""Drop-in for bayesopt/bayesian_optimization.py: ``optimize`` and ``BayesianOptimization``
with the reference's signatures, kwargs, ``state`` dict and return values, running the
inner loop (bayesian_optimization.py:108-247) on the MI355X:

  hyper-parameters   Powell on the host, every MLL evaluation one device call (bo_compute_mll)
  update_k/invert_k  device kernels (bo_update_k, bo_invert_k)
  predict+acquire    ONE fused kernel call (bo_predict_acquire) replacing update_k_star ->
                     update_mean -> update_variance -> standardize_objectives -> update_ucb ->
                     update_hypervolume_improvement -> select_next_batch; the N x M k_star
                     buffer of the reference is never allocated
  evaluation         the user's objective on the host (unchanged)

Multi-GPU (one process per GPU, torch.distributed over RCCL): every rank runs the loop; the
candidate set is sharded over the ranks (distributed.shard_range), each rank scores its shard
and ONE all_gather of the per-rank top-q records selects the batch.  The fit is replicated
(rank 0's hyper-parameters are broadcast), the objective is evaluated on rank 0 and its values
broadcast.

Posterior arrays stay in HBM; callbacks receive a ``state`` dict whose array entries are
copied to numpy only when a callback reads them.
"""

from __future__ import annotations

import time
from typing import Any, Callable, List, Optional, Tuple

import numpy as np
import torch

from . import kernels as K
from .acquisition import (ALL_BATCH_STRATEGIES, MES_BATCH_STRATEGIES, ExclusionMask, _record_indices,
                          check_constraint_bounds,
                          ehvi_select_indices, feasible_rows, hvi_select_indices, mes_select_indices,
                          select_batch_bucb,
                          select_batch_kb, select_batch_ts,
                          select_indices, thompson_draws,
                          update_expected_hypervolume_improvement, update_hypervolume_improvement_exact,
                          update_log_expected_hypervolume_improvement)

ACQUISITIONS = ("sum_ucb", "hvi", "ehvi", "mes", "logehvi")
DEFAULT_MES_SAMPLES = 8


def _check_acquisition(acquisition):
    if acquisition not in ACQUISITIONS:
        raise ValueError(f"unknown acquisition {acquisition!r} (expected 'sum_ucb', 'hvi', 'ehvi', 'mes' "
                         "or 'logehvi')")
from .config import (DEFAULT_BATCH_SIZE, DEFAULT_BETA, DEFAULT_INITIAL_SAMPLES,
                     DEFAULT_LENGTH_SCALE, DEFAULT_PRIOR_MEAN, DEFAULT_PRIOR_VARIANCE,
                     check_fit_method, resolve_float_type)
from .device import F64, require_device
from .pareto import compute_pareto_front, print_pareto_analysis
from .predict import CandidateSet, predict_acquire
from . import _lib


class LazyState(dict):
    """``state`` dict (bayesian_optimization.py:226-243); device arrays become numpy on read."""

    def __getitem__(self, key):
        v = dict.__getitem__(self, key)
        if isinstance(v, torch.Tensor):
            v = v.cpu().numpy()
            dict.__setitem__(self, key, v)
        return v

    def get(self, key, default=None):
        return self[key] if key in self else default

    def items(self):
        return [(k, self[k]) for k in self.keys()]

    def values(self):
        return [self[k] for k in self.keys()]


class DeviceBuffers:
    """The reference's preallocated posterior arrays (bayesian_optimization.py:355-401), in HBM,
    over `m` candidates (this rank's shard).  k_star (n_obj x T x M) is not among them: the fused
    kernel never materialises it."""

    def __init__(self, n_obj, total, m, dev):
        z = lambda *s: torch.zeros(s, dtype=F64, device=dev)  # noqa: E731
        self.kernel_matrices = z(n_obj, total, total)
        self.mu_objectives = z(n_obj, m)
        self.variance_objectives = z(n_obj, m)
        self.std_mu_objectives = z(n_obj, m)
        self.std_variance_objectives = z(n_obj, m)
        self.ucb = z(n_obj, m)
        self.acquisition_values = z(m)


def _world(group=None):
    """(rank, world size) of the torch.distributed group; (0, 1) when not initialised."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(group), dist.get_world_size(group)
    return 0, 1


def _broadcast_np(arr, group=None, device=None):
    """Broadcast a numpy array (or view) from rank 0 in place; a no-op on one rank.  The
    collective's tensor lives where the backend needs it: on `device` (the backend's HIP device,
    default the current one) for RCCL, on the host for gloo."""
    import torch.distributed as dist
    from .distributed import collectives_on
    if not collectives_on(group) or np.size(arr) == 0:
        return arr
    if dist.get_backend(group) == "nccl":
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    else:
        dev = torch.device("cpu")
    t = torch.as_tensor(np.ascontiguousarray(arr, dtype=np.float64), device=dev)
    dist.broadcast(t, 0, group=group)
    arr[...] = t.cpu().numpy().reshape(np.shape(arr))
    return arr


class DeviceBackend:
    """The device side of one loop iteration (bayesian_optimization.py:115-207) on this rank:

      fit      Powell on the device MLL (every evaluation one bo_compute_mll call), rank 0's
               hyper-parameters broadcast, then update_k + invert_k (bo_update_k, bo_invert_k);
      select   the fused predict + acquisition + top-q (bo_predict_acquire) over this rank's
               candidate shard -- the whole set on one rank; shard_range(M, rank, P) and ONE
               all_gather of the 16-B top-q records with P ranks (sharded_predict_acquire) --
               returning the global batch's candidate indices, identical on every rank.

    `state_arrays` gives the callbacks' mu / variance / acquisition arrays over the whole set:
    this rank's buffers, or the shards gathered (a collective: every rank's loop calls it at the
    same point).

    float_type np.float32 (the reference's float32 branch, config.py:54-66): the fit runs COBYLA
    with the float32 jitters (numba_kernels.py:290-302), invert_k adds 1e-3, and the predict runs
    the f32 matrix-core kernel (mode "fp32") with the variance floor 1e-6."""

    def __init__(self, cands, n_obj, total_samples, device=None, buffers=None, group=None, float_type=None,
                 ts_features=1024, ts_seed=0, fit_method="powell", mes_samples=DEFAULT_MES_SAMPLES):
        from .distributed import shard_range
        self.dev = require_device(device)
        self.float_type = resolve_float_type(float_type)
        self.fit_method = check_fit_method(fit_method)
        self.mode = "fp32" if self.float_type == np.float32 else "auto"
        self.cands = cands
        self.group = group
        self.rank, self.world = _world(group)
        self.offset, self.count = shard_range(cands.n, self.rank, self.world)
        if buffers is None:
            buffers = DeviceBuffers(n_obj, total_samples, self.count, self.dev)
        self.bufs = buffers
        self._lu_hint = None           # per objective: the previous invert_k took the LU path
        self.inverse_paths = []
        self._excl_mask = None         # the shard's ExclusionMask (exact-HVI selection)
        # batch_strategy "ts": one generator per backend, drawn from anew every iteration.  Every
        # rank constructs the same generator and draws the same numbers in the same order, so the
        # ranks score the same posterior draws without a collective for them.
        self.ts_features = int(ts_features)
        self._ts_rng = np.random.default_rng(ts_seed)
        # acquisition "mes": the posterior draws behind the sampled maxima come from the same
        # generator, mes_samples of them anew every iteration
        self.mes_samples = int(mes_samples)

    def fit(self, x_vector, y_vector, n, prior_mean, prior_variance, length_scales):
        """Returns (Powell's OptimizeResult, fitted device state, time after the Powell fit)."""
        xd = torch.as_tensor(np.ascontiguousarray(x_vector[:n], dtype=np.float64), device=self.dev)
        yd = torch.as_tensor(np.ascontiguousarray(y_vector[:n], dtype=np.float64), device=self.dev)
        # the default is the reference's fit, called as before; "lbfgs" names itself
        method = {} if self.fit_method == "powell" else {"method": self.fit_method}
        optimized = K.optimize_hyperparams_mll(xd, yd, self.bufs.kernel_matrices, prior_mean,
                                               prior_variance, length_scales, n, float_type=self.float_type,
                                               **method)
        _broadcast_np(length_scales, self.group, self.dev)
        _broadcast_np(prior_variance, self.group, self.dev)
        t1 = time.perf_counter()
        K.update_k(self.bufs.kernel_matrices, xd, 0, n, prior_variance, length_scales)
        # an objective whose Cholesky failed last iteration (Powell-fitted length scales drive
        # cond(K + 1e-6 I) past 1e16) fails again: when all did, go straight to the
        # blocked LU -- gesv's algorithm, the reference's own -- without the doomed attempt
        from .distributed import collectives_on
        if self.world > 1 and collectives_on(self.group):
            kinv = self._invert_split(n)
        else:
            paths = []
            kinv = K.invert_k(n, self.bufs.kernel_matrices, float_type=self.float_type, lu_hint=self._lu_hint,
                              paths=paths)
            self._lu_hint = [p != 0 for p in paths]
            self.inverse_paths = paths
        torch.cuda.synchronize(self.dev)
        return optimized, (xd, yd, kinv), t1

    def _invert_split(self, n):
        """invert_k with the objectives split over the ranks (objective o on rank o mod P), each
        K^-1 then broadcast from its rank (one broadcast per objective: n^2 doubles, 2 MiB at C3).
        Each objective's inverse is the same per-objective device computation as in the batched
        single-rank call, so every rank holds the single-rank K^-1 bit for bit."""
        import torch.distributed as dist
        km = self.bufs.kernel_matrices
        n_obj = km.shape[0]
        mine = [o for o in range(n_obj) if o % self.world == self.rank]
        kinv = torch.empty((n_obj, n, n), dtype=F64, device=self.dev)
        hint = self._lu_hint or [False] * n_obj
        paths = [0] * n_obj
        if mine:
            sub = km[mine] if len(mine) > 1 else km[mine[0]:mine[0] + 1]
            p = []
            got = K.invert_k(n, sub.contiguous(), float_type=self.float_type, lu_hint=[hint[o] for o in mine],
                             paths=p)
            for i, o in enumerate(mine):
                kinv[o] = got[i]
                paths[o] = p[i]
        nccl = dist.get_backend(self.group) == "nccl"
        for o in range(n_obj):
            src = o % self.world                    # a group rank; broadcast takes the global one
            if self.group is not None:
                src = dist.get_global_rank(self.group, src)
            if nccl:
                dist.broadcast(kinv[o], src=src, group=self.group)
            else:                                   # gloo: the collective on a host copy
                h = kinv[o].cpu()
                dist.broadcast(h, src=src, group=self.group)
                kinv[o].copy_(h)
        # the path hints follow the objectives this rank inverts (o mod P is fixed)
        self._lu_hint = [paths[o] != 0 if o in mine else hint[o] for o in range(n_obj)]
        self.inverse_paths = paths
        return kinv

    def _outputs(self):
        b = self.bufs
        return {"mu": b.mu_objectives, "var": b.variance_objectives, "std_mu": b.std_mu_objectives,
                "std_var": b.std_variance_objectives, "ucb": b.ucb, "acq": b.acquisition_values}

    def select(self, fitted, prior_mean, prior_variance, length_scales, betas, batch_size, evaluated,
               acquisition="sum_ucb", y_evaluated=None, reference_point=None, batch_strategy="top",
               constraint_bounds=None):
        """Global candidate indices of the next batch (select_next_batch's order, the evaluated
        points excluded).  "sum_ucb" is the reference's acquisition (acquisition.py:89-108, fused
        top-q); "hvi" replaces the acquisition array with the exact hypervolume improvement of the
        UCB vectors over the Pareto front of `y_evaluated` above `reference_point`; "ehvi" with the
        expected hypervolume improvement of the posterior (mu_objectives, variance_objectives) over
        that front (acquisition.ehvi_select_indices; not in the reference); "mes" with the max-value
        entropy search acquisition over the maxima of `mes_samples` posterior draws
        (acquisition.mes_select_indices; not in the reference; up to 8 objectives, "top" or "gibbon");
        "logehvi" with the natural logarithm of the EHVI (ehvi_select_indices with log=True; not in the
        reference; "top" only): finite and ordered where "ehvi" underflows to 0.0 -- prefer it when the
        length scales are long or the variance sits at its floor.
        batch_strategy "top" is the reference's batch (the batch_size best values of one
        acquisition array); "bucb" (not in the reference) takes every pick after the first from the
        UCB recomputed with the variance conditioned on the earlier picks
        (acquisition.select_batch_bucb), over this process's shard; "ts" (not in the reference)
        takes pick s as the best candidate of posterior draw s (Thompson sampling by pathwise
        conditioning, acquisition.select_batch_ts) for "sum_ucb" and "hvi", with any number of
        ranks: the draws come from this backend's generator (ts_seed), the same on every rank, so no
        collective is needed for them and the exchange of the top-q records merges the shards;
        "kb" (not in the reference; "ehvi" only, one rank) takes every pick after the first from
        the EHVI of the variance conditioned on the earlier picks over the front extended by the
        posterior means at those picks (Kriging believer, acquisition.select_batch_kb);
        "gibbon" (not in the reference; "mes" only, one rank) takes every pick after the first from
        the max-value entropy array plus half the log-ratio of the variance conditioned on the
        earlier picks to the unconditioned one, summed over the objectives (GIBBON's greedy batch
        bound, acquisition.select_batch_gibbon).
        `constraint_bounds` (not in the reference; "ehvi" and "top" only): the last
        len(constraint_bounds) outputs are outcome constraints, y_evaluated carries them after the
        objectives, and the acquisition is the EHVI over the front of the feasible evaluated
        points times the probability of feasibility
        (acquisition.constrained_expected_hypervolume_improvement)."""
        _check_acquisition(acquisition)
        if constraint_bounds is not None:
            _check_constraints(len(prior_mean) - len(constraint_bounds), len(constraint_bounds), constraint_bounds,
                               acquisition, batch_strategy)
        _check_batch_strategy(batch_strategy, acquisition, batch_size, self.group)
        xd, yd, kinv = fitted
        out = self._outputs()
        if batch_strategy == "bucb":
            predict_acquire(xd, yd, kinv, self.cands, prior_mean, prior_variance, length_scales, betas,
                            outputs=tuple(out), topq=0, offset=self.offset, count=self.count, out=out,
                            device=self.dev, mode=self.mode, float_type=self.float_type)
            if self._excl_mask is None:
                self._excl_mask = ExclusionMask(self.cands, self.offset, self.count, self.dev)
            return select_batch_bucb(self.bufs.std_mu_objectives, self.bufs.variance_objectives, xd, kinv,
                                     self.cands, prior_variance, length_scales, betas, evaluated, batch_size,
                                     offset=self.offset, count=self.count, mask=self._excl_mask,
                                     float_type=self.float_type)
        if batch_strategy == "kb":
            predict_acquire(xd, yd, kinv, self.cands, prior_mean, prior_variance, length_scales, betas,
                            outputs=tuple(out), topq=0, offset=self.offset, count=self.count, out=out,
                            device=self.dev, mode=self.mode, float_type=self.float_type)
            if self._excl_mask is None:
                self._excl_mask = ExclusionMask(self.cands, self.offset, self.count, self.dev)
            # acq_out: the callbacks see the EHVI array "top" would show (the first pick's)
            return select_batch_kb(self.bufs.mu_objectives, self.bufs.variance_objectives, xd, kinv, self.cands,
                                   prior_variance, length_scales, y_evaluated, len(y_evaluated), reference_point,
                                   evaluated, batch_size, offset=self.offset, count=self.count,
                                   mask=self._excl_mask, float_type=self.float_type,
                                   acq_out=self.bufs.acquisition_values)
        if batch_strategy == "ts":
            # the predict still runs (topq = 0): the callbacks' state arrays are filled
            predict_acquire(xd, yd, kinv, self.cands, prior_mean, prior_variance, length_scales, betas,
                            outputs=tuple(out), topq=0, offset=self.offset, count=self.count, out=out,
                            device=self.dev, mode=self.mode, float_type=self.float_type)
            if self._excl_mask is None:
                self._excl_mask = ExclusionMask(self.cands, self.offset, self.count, self.dev)
            draws = thompson_draws(self._ts_rng, len(prior_mean), self.cands.dim, xd.shape[0], batch_size,
                                   self.ts_features)
            return select_batch_ts(xd, yd, kinv, self.cands, prior_mean, prior_variance, length_scales, draws,
                                   evaluated, batch_size, acquisition=acquisition, y_evaluated=y_evaluated,
                                   reference_point=reference_point, offset=self.offset, count=self.count,
                                   mask=self._excl_mask, float_type=self.float_type, group=self.group)
        if acquisition == "sum_ucb" and batch_size <= _lib.MAX_TOPQ:
            from .distributed import sharded_predict_acquire
            _, (_, idx) = sharded_predict_acquire(xd, yd, kinv, self.cands, prior_mean, prior_variance,
                                                  length_scales, betas, batch_size, outputs=tuple(out),
                                                  group=self.group, device=self.dev, out=out, mode=self.mode,
                                                  float_type=self.float_type)
            return np.asarray(idx, dtype=np.int64)
        predict_acquire(xd, yd, kinv, self.cands, prior_mean, prior_variance, length_scales, betas,
                        outputs=tuple(out), topq=0, offset=self.offset, count=self.count, out=out,
                        device=self.dev, mode=self.mode, float_type=self.float_type)
        if acquisition == "mes":
            # posterior draws over this shard (anew every iteration, the same on every rank), their
            # maxima over ALL candidates (one all_reduce MAX with several ranks), the scan, the masked
            # top-q, then the fused path's exchange; batches above BO_MAX_TOPQ: the scan only, then
            # the rounds below
            if self._excl_mask is None:
                self._excl_mask = ExclusionMask(self.cands, self.offset, self.count, self.dev)
            draws = thompson_draws(self._ts_rng, len(prior_mean), self.cands.dim, xd.shape[0], self.mes_samples,
                                   self.ts_features)
            if batch_strategy == "gibbon":
                # one rank, batch_size <= BO_MAX_TOPQ (_check_batch_strategy): the scan, then the
                # picks penalised by the variance conditioned on the earlier ones
                return mes_select_indices(self.bufs.acquisition_values, self.bufs.mu_objectives,
                                          self.bufs.variance_objectives, xd, yd, kinv, self.cands, prior_mean,
                                          prior_variance, length_scales, draws, evaluated, batch_size,
                                          offset=self.offset, mask=self._excl_mask, float_type=self.float_type,
                                          group=self.group, batch_strategy="gibbon")
            fits = batch_size <= _lib.MAX_TOPQ
            rec = mes_select_indices(self.bufs.acquisition_values, self.bufs.mu_objectives,
                                     self.bufs.variance_objectives, xd, yd, kinv, self.cands, prior_mean,
                                     prior_variance, length_scales, draws, evaluated, batch_size,
                                     offset=self.offset, return_record=True, mask=self._excl_mask,
                                     float_type=self.float_type, group=self.group, select=fits)
            if fits:
                from .distributed import collectives_on, exchange_topq_rec
                if not collectives_on(self.group):
                    return _record_indices(rec, batch_size)
                return np.asarray(exchange_topq_rec(rec, batch_size, self.group)[1], dtype=np.int64)
        if acquisition in ("hvi", "ehvi", "logehvi") and batch_size <= _lib.MAX_TOPQ:
            # the exact HVI and its top-q with exclusion in one device pass over this shard (the
            # EHVI: its scan, then the masked top-q), then the fused path's exchange
            # the shard's exclusion mask persists across iterations: only the new batch's rows
            # are added to it (ExclusionMask)
            if self._excl_mask is None:
                self._excl_mask = ExclusionMask(self.cands, self.offset, self.count, self.dev)
            if acquisition == "hvi":
                rec = hvi_select_indices(self.bufs.acquisition_values, self.bufs.ucb, y_evaluated,
                                         len(y_evaluated), reference_point, prior_mean, prior_variance,
                                         self.cands, evaluated, batch_size, offset=self.offset,
                                         return_record=True, mask=self._excl_mask)
            else:
                rec = ehvi_select_indices(self.bufs.acquisition_values, self.bufs.mu_objectives,
                                          self.bufs.variance_objectives, y_evaluated, len(y_evaluated),
                                          reference_point, self.cands, evaluated, batch_size,
                                          offset=self.offset, return_record=True, mask=self._excl_mask,
                                          constraint_bounds=constraint_bounds, log=acquisition == "logehvi")
            from .distributed import collectives_on, exchange_topq_rec
            if not collectives_on(self.group):
                return _record_indices(rec, batch_size)
            return np.asarray(exchange_topq_rec(rec, batch_size, self.group)[1], dtype=np.int64)
        if acquisition == "hvi":
            update_hypervolume_improvement_exact(self.bufs.acquisition_values, self.bufs.ucb, y_evaluated,
                                                 len(y_evaluated), reference_point, prior_mean,
                                                 prior_variance)
        if acquisition == "ehvi":
            update_expected_hypervolume_improvement(self.bufs.acquisition_values, self.bufs.mu_objectives,
                                                    self.bufs.variance_objectives, y_evaluated,
                                                    len(y_evaluated), reference_point,
                                                    constraint_bounds=constraint_bounds)
        if acquisition == "logehvi":
            update_log_expected_hypervolume_improvement(self.bufs.acquisition_values, self.bufs.mu_objectives,
                                                        self.bufs.variance_objectives, y_evaluated,
                                                        len(y_evaluated), reference_point,
                                                        constraint_bounds=constraint_bounds)
        # batches above BO_MAX_TOPQ: rounds of the standalone device selection (over the gathered
        # array when sharded)
        from .distributed import collectives_on
        acq = self.bufs.acquisition_values if not collectives_on(self.group) else \
            torch.as_tensor(self.state_arrays()["acquisition_values"], device=self.dev)
        return select_indices(acq, self.cands, evaluated, batch_size)

    def state_arrays(self):
        b = self.bufs
        arrs = {"mu_objectives": b.mu_objectives, "variance_objectives": b.variance_objectives,
                "acquisition_values": b.acquisition_values}
        from .distributed import collectives_on, gather_shards
        if not collectives_on(self.group):
            return arrs
        return {k: gather_shards(v, self.cands.n, self.group) for k, v in arrs.items()}


def optimize(x_vector, y_vector, kernel_matrices, k_star, mu_objectives, variance_objectives,
             std_mu_objectives, std_variance_objectives, ucb, acquisition_values, input_space,
             prior_mean, prior_variance, reference_point, n_evaluations, total_samples,
             n_objectives, function, betas, length_scales, batch_size, bounds,
             callbacks: Optional[List[Callable]] = None, *,
             acquisition: str = "sum_ucb", group=None, backend=None,
             float_type=None, batch_strategy: str = "top", ts_features: int = 1024,
             ts_seed: int = 0, constraint_bounds=None, fit_method: str = "powell",
             mes_samples: int = DEFAULT_MES_SAMPLES) -> Tuple[np.ndarray, np.ndarray, int]:
    """bayesian_optimization.py:51-247 with the reference's argument list.

    `kernel_matrices` and the posterior arrays may be HIP tensors (in place) or numpy arrays;
    `k_star` is accepted for signature compatibility and not used (nothing N x M is
    materialised); `input_space` may be a CandidateSet, a device tensor or the reference's
    int64 numpy array.  Returns (x_vector, y_vector, last_eval + 1) like the reference
    (including its count quirk, :247).

    With torch.distributed initialised (one process per GPU) every rank runs this loop over its
    shard of the candidates (module docstring); the posterior arrays given here are then not
    filled (each rank holds its shard), the state dict's arrays are the gathered whole.  `group`
    selects the process group; `backend` replaces the device side (DeviceBackend's interface:
    fit / select / state_arrays / cands / rank / world / bufs).  `float_type` np.float32 runs the
    reference's float32 branch (DeviceBackend).  `batch_strategy` "bucb" selects each batch by
    hallucinated observations (DeviceBackend.select; one rank, acquisition "sum_ucb",
    batch_size <= BO_MAX_TOPQ); "ts" by Thompson sampling over pathwise posterior draws
    (acquisition "sum_ucb" or "hvi", any number of ranks, batch_size <= BO_MAX_TOPQ), with
    `ts_features` random Fourier features and the draws of default_rng(`ts_seed`) -- every rank
    constructs the same generator, so no collective is needed for the draws (both are the
    backend's when `backend` is given); "kb" by a Kriging believer for the EHVI (acquisition "ehvi"
    only, one rank, batch_size <= BO_MAX_TOPQ): each pick joins the front as a believed observation
    equal to the posterior mean; "top", the default, is the reference's batch.
    `constraint_bounds` (n_con pairs (lo, hi); acquisition "ehvi" and batch_strategy "top" only):
    the last n_con of the len(prior_mean) outputs are outcome constraints -- `function` returns
    them after the objectives, y_vector and the posterior arrays carry them as further columns /
    rows, reference_point has one coordinate per objective -- and the acquisition is the EHVI over
    the front of the feasible evaluated points times the probability of feasibility
    (DeviceBackend.select).
    `fit_method` "lbfgs" fits the length scales by L-BFGS-B over log ls with the device's analytic
    MLL gradient (kernels.optimize_hyperparams_mll, method="lbfgs": prior_variance stays as given);
    "powell", the default, is the reference's fit.  It is the backend's when `backend` is given.
    `acquisition` "logehvi" (not in the reference; what "ehvi" takes, batch_strategy "top" only, outcome
    constraints included) is the EHVI in log space (acquisition.log_expected_hypervolume_improvement):
    prefer it to "ehvi" when the length scales are long or the variance sits at its floor, where "ehvi"
    is exactly 0.0 at most candidates and a batch is completed in index order.
    `acquisition` "mes" (not in the reference; 1 to 8 objectives, batch_strategy "top" with any
    number of ranks, or "gibbon" on one rank) is the max-value entropy search acquisition
    (acquisition.max_value_entropy) over the maxima of `mes_samples` posterior draws
    (1 .. BO_MAX_TOPQ, default 8; drawn anew every iteration from default_rng(`ts_seed`) with
    `ts_features` features, the same on every rank; the backend's when `backend` is given).
    `batch_strategy` "gibbon" (acquisition "mes" only, one rank, batch_size <= BO_MAX_TOPQ) computes
    that array once and takes every pick after the first from it plus GIBBON's batch correction,
    half the log-ratio of the variance conditioned on the earlier picks to the unconditioned one
    summed over the objectives (acquisition.select_batch_gibbon): the batch spreads instead of
    crowding one maximum.

    Callbacks with several ranks: the state arrays are the shards gathered, a collective; whether
    to gather is decided once, collectively (any rank with callbacks), so that a callback
    registered on rank 0 only keeps every rank's collectives matched.
    """
    del k_star, n_objectives, bounds  # unused, as in the reference (reference_point too, unless
    #                                   acquisition="hvi" / "ehvi", the exact / expected hypervolume improvement)
    n_obj = len(prior_mean)
    if constraint_bounds is not None:
        _check_constraints(n_obj - len(constraint_bounds), len(constraint_bounds), constraint_bounds, acquisition,
                           batch_strategy)
    _check_batch_strategy(batch_strategy, acquisition, batch_size, getattr(backend, "group", group))
    if acquisition == "mes":
        _check_mes_samples(getattr(backend, "mes_samples", mes_samples))
    if backend is None:
        dev = require_device()
        cands = input_space if isinstance(input_space, CandidateSet) else CandidateSet.explicit(input_space, dev)
        from .distributed import shard_range
        _, world = _world(group)
        cnt = shard_range(cands.n, _world(group)[0], world)[1]

        def dev_buf(a, shape):
            if isinstance(a, torch.Tensor) and a.device.type == "cuda" and tuple(a.shape) == shape:
                return a
            return torch.zeros(shape, dtype=F64, device=dev)

        bufs = DeviceBuffers.__new__(DeviceBuffers)
        bufs.kernel_matrices = dev_buf(kernel_matrices, (n_obj, total_samples, total_samples))
        bufs.mu_objectives = dev_buf(mu_objectives, (n_obj, cnt))
        bufs.variance_objectives = dev_buf(variance_objectives, (n_obj, cnt))
        bufs.std_mu_objectives = dev_buf(std_mu_objectives, (n_obj, cnt))
        bufs.std_variance_objectives = dev_buf(std_variance_objectives, (n_obj, cnt))
        bufs.ucb = dev_buf(ucb, (n_obj, cnt))
        bufs.acquisition_values = dev_buf(acquisition_values, (cnt,))
        backend = DeviceBackend(cands, n_obj, total_samples, dev, bufs, group, float_type=float_type,
                                ts_features=ts_features, ts_seed=ts_seed, fit_method=fit_method,
                                mes_samples=mes_samples)
    cands, rank, world = backend.cands, backend.rank, backend.world
    gather = bool(callbacks)
    bgroup = getattr(backend, "group", group)
    from .distributed import collectives_on
    coll = collectives_on(bgroup)
    if coll:                            # any rank with callbacks: every rank joins the gathers
        import torch.distributed as dist
        if dist.get_backend(bgroup) == "nccl":      # RCCL: the flag on the backend's HIP device
            bdev = getattr(backend, "dev", None)
            fdev = torch.device(bdev) if bdev is not None else torch.device("cuda", torch.cuda.current_device())
        else:
            fdev = torch.device("cpu")
        flag = torch.tensor([1.0 if callbacks else 0.0], dtype=torch.float64, device=fdev)
        dist.all_reduce(flag, op=dist.ReduceOp.MAX, group=bgroup)
        gather = bool(flag.item())

    last_eval = 0
    for current_eval in range(n_evaluations, total_samples, batch_size):
        iter_start = time.perf_counter()
        t0 = time.perf_counter()
        optimized, fitted, t1 = backend.fit(x_vector, y_vector, current_eval, prior_mean, prior_variance,
                                            length_scales)
        t2 = time.perf_counter()
        # the default strategy is not passed on: a caller's backend keeps the interface it has
        strat = {} if batch_strategy == "top" else {"batch_strategy": batch_strategy}
        if constraint_bounds is not None:   # likewise, only when set
            strat["constraint_bounds"] = constraint_bounds
        idx = backend.select(fitted, prior_mean, prior_variance, length_scales, betas, batch_size,
                             x_vector[:current_eval], acquisition, y_vector[:current_eval], reference_point,
                             **strat)
        x_next = cands.points(idx) if idx.size else np.zeros((0, cands.dim), dtype=np.int64)
        t3 = time.perf_counter()
        for b_idx, point in enumerate(x_next):
            x_vector[current_eval + b_idx] = point
            if rank == 0:       # the user's objective, once per point (bayesian_optimization.py:213-216)
                y_vector[current_eval + b_idx] = function(point)
        if coll:
            _broadcast_np(y_vector[current_eval:current_eval + len(x_next)], bgroup,
                          getattr(backend, "dev", None))
        last_eval = current_eval
        t4 = time.perf_counter()
        if gather:
            arrs = backend.state_arrays()
        if callbacks:
            state = LazyState({
                "iteration": current_eval,
                "n_evaluations": current_eval + batch_size,
                "x_vector": x_vector[: current_eval + batch_size],
                "y_vector": y_vector[: current_eval + batch_size],
                "mu_objectives": arrs["mu_objectives"],
                "variance_objectives": arrs["variance_objectives"],
                "acquisition_values": arrs["acquisition_values"],
                "x_next": x_next,
                "hyperparams": optimized.x,
                # the reference's keys; update_k_star (its "kernels", :145-153) is fused into the
                # predict call and so counted under "acquisition" here
                "timings": {"hyperparams": t1 - t0, "kernels": t2 - t1, "acquisition": t3 - t2,
                            "eval": t4 - t3, "total": t4 - iter_start},
            })
            for cb in callbacks:
                cb(state)
    bufs = getattr(backend, "bufs", None)
    if bufs is not None and world == 1:
        if isinstance(kernel_matrices, np.ndarray):   # the reference mutates it in place (update_k)
            kernel_matrices[...] = bufs.kernel_matrices.cpu().numpy().reshape(kernel_matrices.shape)
        for name, a in (("mu", mu_objectives), ("var", variance_objectives), ("smu", std_mu_objectives),
                        ("svar", std_variance_objectives), ("ucb", ucb), ("acq", acquisition_values)):
            if isinstance(a, np.ndarray):   # numpy callers get their arrays filled, as in the reference
                src = {"mu": bufs.mu_objectives, "var": bufs.variance_objectives,
                       "smu": bufs.std_mu_objectives, "svar": bufs.std_variance_objectives,
                       "ucb": bufs.ucb, "acq": bufs.acquisition_values}[name]
                a[...] = src.cpu().numpy()
    return x_vector, y_vector, last_eval + 1


def _check_batch_strategy(batch_strategy, acquisition, batch_size, group=None):
    """What batch_strategy="bucb" / "ts" / "kb" / "gibbon" do not cover raises here, with the reason."""
    if batch_strategy not in ALL_BATCH_STRATEGIES + MES_BATCH_STRATEGIES:
        raise ValueError(f"unknown batch_strategy {batch_strategy!r} (expected 'top', 'bucb' or 'ts', "
                         "or 'kb' with acquisition='ehvi'), or 'gibbon' with acquisition='mes'")
    if batch_strategy == "gibbon":
        if acquisition != "mes":
            raise ValueError("batch_strategy='gibbon' adds half the log-ratio of the conditioned to the "
                             "unconditioned variance: the penalty is the batch correction of an information "
                             f"criterion, defined for acquisition='mes' only (got acquisition={acquisition!r})")
        if batch_size > _lib.MAX_TOPQ:
            raise ValueError(f"batch_strategy='gibbon' supports batch_size <= {_lib.MAX_TOPQ} (got {batch_size})")
        from .distributed import collectives_on
        if collectives_on(group):
            raise ValueError("batch_strategy='gibbon' runs on one rank: with several, every pick would need an "
                             "all-gather of the per-rank best candidates")
        return
    if acquisition == "mes" and batch_strategy != "top":
        why = {"bucb": "'bucb' conditions the UCB acquisition ('sum_ucb')",
               "ts": "'ts' scores one posterior draw per pick, and 'mes' already averages over its draws' maxima: "
                     "it has no per-draw form",
               "kb": "'kb' extends the EHVI's front by believed observations"}[batch_strategy]
        raise ValueError(f"acquisition='mes' supports batch_strategy='top' only (got {batch_strategy!r}): {why}; "
                         "a batch for the max-value entropy would need the variance conditioned on the earlier picks "
                         "(batch_strategy='gibbon' is that batch)")
    if acquisition == "logehvi" and batch_strategy != "top":
        why = {"bucb": "'bucb' conditions the UCB acquisition ('sum_ucb')",
               "ts": "'ts' scores posterior draws, and the EHVI integrates over the posterior: it has no sampled form",
               "kb": "'kb' (Kriging believer) integrates the linear EHVI while it selects; a believer over the log "
                     "value is not built (use acquisition='ehvi' with 'kb')"}[batch_strategy]
        raise ValueError(f"acquisition='logehvi' supports batch_strategy='top' only (got {batch_strategy!r}): {why}")
    if batch_strategy == "kb":
        if acquisition != "ehvi":
            raise ValueError("batch_strategy='kb' (Kriging believer) extends the front by believed observations: "
                             f"it is defined for acquisition='ehvi' only (got acquisition={acquisition!r})")
        if batch_size > _lib.MAX_TOPQ:
            raise ValueError(f"batch_strategy='kb' supports batch_size <= {_lib.MAX_TOPQ} (got {batch_size})")
        from .distributed import collectives_on
        if collectives_on(group):
            raise ValueError("batch_strategy='kb' runs on one rank: with several, every pick would need an "
                             "all-gather of the per-rank best candidates and of the believed vector")
        return
    if batch_strategy == "ts":
        if acquisition not in ("sum_ucb", "hvi"):
            raise ValueError("batch_strategy='ts' scores posterior draws; acquisition='ehvi' integrates over "
                             f"the posterior and has no sampled form (got acquisition={acquisition!r})")
        if batch_size > _lib.MAX_TOPQ:
            raise ValueError(f"batch_strategy='ts' supports batch_size <= {_lib.MAX_TOPQ} (got {batch_size})")
        return
    if batch_strategy != "bucb":
        return
    if acquisition != "sum_ucb":
        raise ValueError("batch_strategy='bucb' conditions the UCB acquisition ('sum_ucb'); it is not defined "
                         f"for acquisition={acquisition!r}")
    if batch_size > _lib.MAX_TOPQ:
        raise ValueError(f"batch_strategy='bucb' supports batch_size <= {_lib.MAX_TOPQ} (got {batch_size})")
    from .distributed import collectives_on
    if collectives_on(group):
        raise ValueError("batch_strategy='bucb' runs on one rank: with several, every pick would need an "
                         "all-gather of the per-rank best candidates")


def _check_constraints(n_obj, n_con, constraint_bounds, acquisition, batch_strategy):
    """What outcome constraints do not cover raises here, with the reason; then the bounds' own
    rules (acquisition.check_constraint_bounds)."""
    if n_con < 0:
        raise ValueError(f"n_constraints must be >= 0 (got {n_con})")
    if n_con == 0 and constraint_bounds is None:
        return
    if acquisition not in ("ehvi", "logehvi"):
        why = {"sum_ucb": "'sum_ucb' takes negative values, so its product with a probability of feasibility "
                          "does not order the candidates",
               "hvi": "'hvi' scores UCB vectors, not a posterior that a probability of feasibility could weight"}
        raise ValueError("outcome constraints need acquisition='ehvi': "
                         f"{why.get(acquisition, repr(acquisition) + ' has no constrained form')}")
    if batch_strategy != "top":
        why = {"kb": "'kb' would have to condition the constraint GPs on the believed point and decide its "
                     "feasibility",
               "ts": "'ts' would have to sample the constraint GPs",
               "bucb": "'bucb' is not defined for the EHVI"}
        raise ValueError("outcome constraints need batch_strategy='top': "
                         f"{why.get(batch_strategy, repr(batch_strategy) + ' has no constrained form')}")
    if not 1 <= n_obj <= 4:
        raise ValueError(f"outcome constraints need 1 <= n_objectives <= 4 (got {n_obj}): the expected "
                         "hypervolume improvement's box decomposition is limited to n_obj <= 4")
    if n_obj + n_con > _lib.MAX_OBJ:
        raise ValueError(f"n_objectives + n_constraints must be <= {_lib.MAX_OBJ} (got {n_obj} + {n_con}): "
                         "every output has its own GP in one predict call")
    check_constraint_bounds(constraint_bounds, n_con)


def _check_mes_samples(mes_samples):
    if not 1 <= int(mes_samples) <= _lib.MAX_TOPQ:
        raise ValueError(f"mes_samples must be in [1, {_lib.MAX_TOPQ}] (got {mes_samples}): the posterior draws "
                         "of one bo_sample_paths call")


def _check_limits(n_obj, dim, total_samples, batch_size, acquisition="sum_ucb", batch_strategy="top", group=None,
                  n_constraints=0, constraint_bounds=None, fit_method="powell", mes_samples=DEFAULT_MES_SAMPLES):
    """Fail in the constructor -- before any objective evaluation -- on shapes the device path
    cannot run (the reference would hit them only mid-loop, if at all).  n_obj counts the
    objectives; the n_constraints outcome constraints are further outputs."""
    check_fit_method(fit_method)
    _check_constraints(n_obj, n_constraints, constraint_bounds, acquisition, batch_strategy)
    _check_batch_strategy(batch_strategy, acquisition, batch_size, group)
    if acquisition == "mes":
        _check_mes_samples(mes_samples)
    if not 1 <= n_obj <= _lib.MAX_OBJ:
        raise ValueError(f"n_objectives must be in [1, {_lib.MAX_OBJ}] (got {n_obj})")
    if acquisition == "hvi" and n_obj > 4:
        raise ValueError(f"acquisition='hvi' supports at most 4 objectives (got {n_obj}): the exact "
                         "hypervolume improvement's box decomposition is limited to n_obj <= 4")
    if acquisition == "ehvi" and n_obj > 4:
        raise ValueError(f"acquisition='ehvi' supports at most 4 objectives (got {n_obj}): the expected "
                         "hypervolume improvement's box decomposition is limited to n_obj <= 4")
    if acquisition == "logehvi" and n_obj > 4:
        raise ValueError(f"acquisition='logehvi' supports at most 4 objectives (got {n_obj}): the expected "
                         "hypervolume improvement's box decomposition is limited to n_obj <= 4")
    if not 1 <= dim <= _lib.MAX_DIM:
        raise ValueError(f"the input dimension must be in [1, {_lib.MAX_DIM}] (got {dim})")
    if batch_size < 1:
        raise ValueError("batch_size must be >= 1")
    d = _lib.PredictDesc()
    n_out = n_obj + n_constraints
    d.n_obj, d.dim, d.n_train, d.n_cand, d.cand_kind, d.topq = n_out, dim, total_samples, 1, _lib.CAND_GRID, 0
    for k in range(dim):
        d.grid_shape[k] = 1
    lib = _lib.load()
    if lib.bo_predict_workspace_size(d) == 0 or lib.bo_invert_k_workspace_size(n_out, total_samples) == 0:
        raise ValueError(f"total_samples = {total_samples} exceeds the device path's limits "
                         f"(predict: N <= 16384 and n_obj N^2 doubles < 2 GiB)")


class BayesianOptimization:
    """bayesian_optimization.py:250-488 — same constructor, kwargs and methods.

    Extra kwargs (not in the reference): ``input_space`` (explicit [M, d] candidates, e.g.
    a Sobol set, or a CandidateSet such as CandidateSet.sobol_set(...), instead of the integer
    grid), ``device``, ``acquisition`` ("sum_ucb", the reference's default; "hvi": exact
    hypervolume improvement of the UCB vectors over the evaluated Pareto front; or "ehvi": the
    expected hypervolume improvement of the posterior over that front, objectives independent; or
    "logehvi": the natural logarithm of the EHVI, acquisition.log_expected_hypervolume_improvement, for what
    "ehvi" takes with batch_strategy "top" -- prefer it where "ehvi" underflows to 0.0 (long length scales, the
    variance at its floor); or
    "mes": max-value entropy search, acquisition.max_value_entropy, for 1 to 8 objectives and
    batch_strategy "top" or "gibbon", over the maxima of ``mes_samples`` posterior draws, default 8, drawn anew
    every iteration from the ``ts_seed`` generator with ``ts_features`` features),
    ``reference_point`` (the HVI reference point; the reference fixes it at zeros and never uses
    it, bayesian_optimization.py:425), ``group`` (the torch.distributed process group of a
    multi-GPU run; default: the world when initialised), ``float_type`` (np.float64, the default
    of config.NUMBA_FLOAT_TYPE, or np.float32: the reference's float32 branch -- config.py:54-66
    jitters and variance floor, COBYLA for the fit, float32 host arrays -- with the predict on the
    f32 matrix cores) and ``initial_points`` ([n0, d] points evaluated as the initial design
    instead of the Latin hypercube) and ``batch_strategy`` ("top", the reference's batch: the
    batch_size best acquisition values; or "bucb": every pick after the first accounts for the
    earlier ones through hallucinated observations, acquisition.select_batch_bucb; or "ts": pick s
    is the best candidate of posterior draw s, acquisition.select_batch_ts, with ``ts_features``
    random Fourier features, default 1024, and the draws of numpy.random.default_rng(``ts_seed``),
    default 0 -- every rank constructs the same generator and draws anew every iteration, so the
    ranks need no collective for the draws; or "kb", with acquisition "ehvi" only: a Kriging
    believer, every pick after the first maximises the EHVI of the variance conditioned on the
    earlier picks over the front extended by the posterior means there,
    acquisition.select_batch_kb; or "gibbon", with acquisition "mes" only: every pick after the first
    maximises the max-value entropy array plus half the log-ratio of the variance conditioned on
    the earlier picks to the unconditioned one, GIBBON's greedy batch bound,
    acquisition.select_batch_gibbon), and ``n_constraints`` with ``constraint_bounds`` (outcome
    constraints, acquisition "ehvi" and batch_strategy "top" only: ``function`` returns
    n_objectives + n_constraints values, the objectives first; constraint j is feasible inside
    constraint_bounds[j] = (lo, hi), either infinite on its own side; y_vector has
    n_objectives + n_constraints columns and prior_mean / prior_variance / length_scales / betas
    that length, reference_point has length n_objectives; the acquisition is the EHVI over the
    front of the feasible evaluated points times the probability of feasibility, and
    pareto_analysis reports the feasible front over the objective columns), and ``fit_method``
    ("powell", the reference's fit; or "lbfgs": L-BFGS-B over log(length scale) with the device's
    analytic MLL gradient, kernels.optimize_hyperparams_mll -- every output's GP is fitted the same
    way, prior_variance stays as computed from the initial design, and rank 0's result is broadcast
    as the Powell fit's is).
    With several ranks, each holds its shard of the posterior arrays, the initial design is drawn
    and evaluated on rank 0 (every rank draws the same RNG numbers, so the RNG stays in step) and
    broadcast, and the loop runs as `optimize` describes.
    """

    def __init__(self, function: Callable[[np.ndarray], np.ndarray], bounds: List[Tuple[int, int]],
                 n_objectives: int = 3, n_iterations: int = 10, **kwargs: Any):
        self.device = require_device(kwargs.get("device"))
        self.group = kwargs.get("group")
        self.float_type = resolve_float_type(kwargs.get("float_type"))
        ft = self.float_type
        self.function = function
        self.bounds = bounds
        self.n_objectives = n_objectives
        self.n_iterations = n_iterations
        cb = kwargs.get("callbacks", None)
        self.callbacks = [] if cb is None else (cb if isinstance(cb, list) else [cb])
        self.n_constraints = int(kwargs.get("n_constraints", 0))
        self.constraint_bounds = kwargs.get("constraint_bounds")
        if self.n_constraints == 0 and self.constraint_bounds is not None and len(self.constraint_bounds) == 0:
            self.constraint_bounds = None
        n_out = n_objectives + max(self.n_constraints, 0)     # the GPs: objectives, then constraints
        self.prior_mean = np.array(kwargs.get("prior_mean", [DEFAULT_PRIOR_MEAN] * n_out), dtype=ft)
        self.prior_variance = np.array(kwargs.get("prior_variance", [DEFAULT_PRIOR_VARIANCE] * n_out), dtype=ft)
        self.length_scales = np.array(kwargs.get("length_scales", [DEFAULT_LENGTH_SCALE] * n_out), dtype=ft)
        self.betas = np.array(kwargs.get("betas", [DEFAULT_BETA] * n_out), dtype=ft)
        self.batch_size = kwargs.get("batch_size", DEFAULT_BATCH_SIZE)
        init_pts = kwargs.get("initial_points")
        if init_pts is not None:
            init_pts = np.asarray(init_pts)
            if init_pts.ndim != 2 or init_pts.shape[1] != len(bounds):
                raise ValueError("initial_points must be [n0, len(bounds)]")
        self.initial_samples = init_pts.shape[0] if init_pts is not None else \
            kwargs.get("initial_samples", DEFAULT_INITIAL_SAMPLES)
        self.dim = len(bounds)
        explicit = kwargs.get("input_space")
        if explicit is None:
            self.candidates = CandidateSet.grid(bounds)
        elif isinstance(explicit, CandidateSet):
            self.candidates = explicit
        else:
            self.candidates = CandidateSet.explicit(explicit, self.device)
        self._input_space = None
        self.total_samples = self.initial_samples + self.n_iterations * self.batch_size
        self.acquisition = kwargs.get("acquisition", "sum_ucb")
        _check_acquisition(self.acquisition)
        self.batch_strategy = kwargs.get("batch_strategy", "top")
        self.ts_features = int(kwargs.get("ts_features", 1024))
        self.ts_seed = kwargs.get("ts_seed", 0)
        if not 1 <= self.ts_features <= _lib.TS_MAX_FEATURES:
            raise ValueError(f"ts_features must be in [1, {_lib.TS_MAX_FEATURES}] (got {self.ts_features})")
        self.fit_method = kwargs.get("fit_method", "powell")
        self.mes_samples = kwargs.get("mes_samples", DEFAULT_MES_SAMPLES)
        _check_limits(n_objectives, self.dim, self.total_samples, self.batch_size, self.acquisition,
                      self.batch_strategy, self.group, self.n_constraints, self.constraint_bounds, self.fit_method,
                      self.mes_samples)
        self.reference_point = np.array(kwargs.get("reference_point", [0.0] * n_objectives), dtype=ft)
        if self.constraint_bounds is not None:
            self.constraint_bounds = check_constraint_bounds(self.constraint_bounds, self.n_constraints)
            for name in ("prior_mean", "prior_variance", "length_scales", "betas"):
                if len(getattr(self, name)) != n_out:
                    raise ValueError(f"{name} must have one entry per output, n_objectives + n_constraints = "
                                     f"{n_out} (got {len(getattr(self, name))})")
            if len(self.reference_point) != n_objectives:
                raise ValueError("reference_point must have one coordinate per objective, n_objectives = "
                                 f"{n_objectives} (got {len(self.reference_point)}): constraints have none")
        self.x_vector = np.zeros((self.total_samples, self.dim), dtype=ft)
        self.y_vector = np.zeros((self.total_samples, n_out), dtype=ft)
        self._backend = DeviceBackend(self.candidates, n_out, self.total_samples, self.device,
                                      group=self.group, float_type=ft, ts_features=self.ts_features,
                                      ts_seed=self.ts_seed, fit_method=self.fit_method,
                                      mes_samples=self.mes_samples)
        self._buffers = self._backend.bufs
        self.k_star = None   # never materialised (the reference allocates n_obj x T x M here)
        rank, world = _world(self.group)
        # the objective runs on rank 0 only; the other ranks draw the same LHS numbers (their RNG
        # stays in step with rank 0's) and receive rank 0's design and values
        fn = self.function if rank == 0 else (lambda _p: np.zeros(n_out))
        if init_pts is not None:
            for i in range(self.initial_samples):
                self.x_vector[i] = init_pts[i]
                self.y_vector[i] = fn(self.x_vector[i])
            self.n_evaluations = self.initial_samples
        else:
            self.n_evaluations = K.initialize_lhs_integer(self.x_vector, self.y_vector,
                                                          np.array(self.bounds, dtype=np.int64),
                                                          fn, self.initial_samples)
        _broadcast_np(self.x_vector[: self.n_evaluations], self.group, self.device)
        _broadcast_np(self.y_vector[: self.n_evaluations], self.group, self.device)
        if np.all(self.prior_mean == DEFAULT_PRIOR_MEAN):
            self.prior_mean = K.compute_prior_mean(self.y_vector, self.n_evaluations, n_out).astype(ft)
        if np.all(self.prior_variance == DEFAULT_PRIOR_VARIANCE):
            self.prior_variance = K.compute_prior_variance(self.y_vector, self.n_evaluations,
                                                           n_out).astype(ft)

    # the reference's preallocated arrays, materialised on the host on demand
    @property
    def input_space(self):
        if self._input_space is None:
            self._input_space = self.candidates.materialize(self.device).cpu().numpy()
        return self._input_space

    def _np(self, name):
        return getattr(self._buffers, name).cpu().numpy()

    kernel_matrices = property(lambda self: self._np("kernel_matrices"))
    mu_objectives = property(lambda self: self._np("mu_objectives"))
    variance_objectives = property(lambda self: self._np("variance_objectives"))
    std_mu_objectives = property(lambda self: self._np("std_mu_objectives"))
    std_variance_objectives = property(lambda self: self._np("std_variance_objectives"))
    ucb = property(lambda self: self._np("ucb"))
    acquisition_values = property(lambda self: self._np("acquisition_values"))

    def optimize(self) -> None:
        """bayesian_optimization.py:427-463."""
        b = self._buffers
        self.x_vector, self.y_vector, self.n_evaluations = optimize(
            x_vector=self.x_vector, y_vector=self.y_vector, kernel_matrices=b.kernel_matrices,
            k_star=None, mu_objectives=b.mu_objectives, variance_objectives=b.variance_objectives,
            std_mu_objectives=b.std_mu_objectives, std_variance_objectives=b.std_variance_objectives,
            ucb=b.ucb, acquisition_values=b.acquisition_values, input_space=self.candidates,
            prior_mean=self.prior_mean, prior_variance=self.prior_variance,
            reference_point=self.reference_point, n_evaluations=self.n_evaluations,
            total_samples=self.total_samples, n_objectives=self.n_objectives, function=self.function,
            betas=self.betas, length_scales=self.length_scales, batch_size=self.batch_size,
            bounds=self.bounds, callbacks=self.callbacks if self.callbacks else None,
            acquisition=self.acquisition, group=self.group, backend=self._backend,
            float_type=self.float_type, batch_strategy=self.batch_strategy, ts_features=self.ts_features,
            ts_seed=self.ts_seed, constraint_bounds=self.constraint_bounds, fit_method=self.fit_method,
            mes_samples=self.mes_samples)

    def pareto_analysis(self) -> np.ndarray:
        """bayesian_optimization.py:465-488.  With outcome constraints: the front of the feasible
        evaluated points (acquisition.feasible_rows) over the objective columns."""
        ey = self.y_vector[: self.n_evaluations]
        ex = self.x_vector[: self.n_evaluations]
        if self.constraint_bounds is not None:
            ok = feasible_rows(ey, self.n_objectives, self.constraint_bounds)
            ex, ey = ex[ok], np.ascontiguousarray(ey[ok][:, : self.n_objectives])
        px, py = compute_pareto_front(ex, ey)
        print_pareto_analysis(px, py)
        return py

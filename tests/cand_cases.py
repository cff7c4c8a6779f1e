"""One shard of a candidate set in every form the library accepts, for the consumers of the shared
candidate decode (csrc/bo_cand.h): the implicit form -- a grid or the Sobol sequence, decoded on
the device from the global index -- and the same rows as explicit int64 / f64 arrays.  The decode
has no reference but itself in another form, so the forms' outputs are compared bit for bit
(tests/test_gpu_cand_decode.py) and digested for a comparison between two builds of the library
(scripts/cand_outputs_sha.py).  An explicit form holds the shard's rows only: its offset is 0 and
the indices it returns are local, which the runners below make of every form's.

The grids: a 32-bit decode; a 64-bit one whose last axis is above 2^31 and whose shard crosses a
row boundary; a 64-bit one of odd dimension (a padded coordinate) whose shard crosses into the next
index of both leading axes."""
import functools

import numpy as np

N_TRAIN, Q, COUNT, N_OBJ = 37, 3, 4000, 2
GRIDS = {
    "grid32": dict(lo=(-5, 100), shape=(70, 90), offset=1234, ls=(6.0, 9.0)),
    "grid64": dict(lo=(-1, 10), shape=(3, 2 ** 31 + 7), offset=2 ** 31 + 7 - 2000, ls=(150.0, 400.0)),
    "grid64_odd": dict(lo=(4, -2, 0), shape=(2, 3, 2 ** 31 + 1), offset=3 * (2 ** 31 + 1) - 1500, ls=(150.0, 400.0)),
}
CASES = tuple(GRIDS) + ("sobol6",)


@functools.lru_cache(maxsize=None)
def case(name):
    """The shard's rows, a fitted state of N_TRAIN of them and the inputs of every consumer (host
    arrays, built once and not modified)."""
    import bayesopt_smart_amd as bo
    from bayesopt_smart_amd.acquisition import thompson_draws
    CS = bo.predict.CandidateSet
    rng = np.random.default_rng(11 + CASES.index(name))
    if name == "sobol6":
        implicit, offset, ls = CS.sobol_set(6, 1 << 20, lo=-2.0, scale=40.0, bits=30), 70_001, (15.0, 25.0)
    else:
        g = GRIDS[name]
        implicit, offset, ls = CS.grid([(l, l + s) for l, s in zip(g["lo"], g["shape"])]), g["offset"], g["ls"]
    rows = implicit.points(offset + np.arange(COUNT))         # int64 for a grid: every value below 2^53
    pts = rows.astype(np.float64)
    if name != "sobol6":
        assert (rows[0, :-1] != rows[-1, :-1]).all()              # the shard crosses every leading axis
    x = pts[rng.choice(COUNT, N_TRAIN, replace=False)]
    pv, ls = np.array([1.5, 0.7]), np.array(ls)
    sq = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    kinv = np.stack([np.linalg.inv(pv[o] * np.exp(-0.5 * sq / ls[o] ** 2) + 1e-6 * np.eye(N_TRAIN))
                     for o in range(N_OBJ)])
    y = rng.standard_normal((N_TRAIN, N_OBJ))
    pm = y.mean(0)
    smu = rng.standard_normal((N_OBJ, COUNT))
    var = pv[:, None] * rng.uniform(0.2, 1.0, (N_OBJ, COUNT))
    acq = rng.standard_normal(COUNT)
    hot = rng.choice(COUNT, 40, replace=False)
    acq[hot] = 30.0 + np.arange(40)                           # the top of the order: evaluated points
    miss = pts[:5].copy()
    miss[:, 0] += 0.5                                         # equal to no candidate
    return dict(name=name, implicit=implicit, offset=offset, rows=rows, pts=pts, x=x, y=y, kinv=kinv, pm=pm, pv=pv,
                ls=ls, beta=np.array([2.0, 1.5]), smu=smu, var=var, mu=pm[:, None] + np.sqrt(pv)[:, None] * smu,
                acq=acq, hot=hot, ev=np.concatenate([pts[hot], x, miss]),
                draws=thompson_draws(np.random.default_rng(5), N_OBJ, pts.shape[1], N_TRAIN, Q, 64))


def forms(c):
    """(label, candidate set, offset of the shard in it): the implicit form first."""
    import bayesopt_smart_amd as bo
    CS = bo.predict.CandidateSet
    out = [(c["implicit"].kind, c["implicit"], c["offset"]), ("f64", CS.explicit(c["pts"], "cuda"), 0)]
    if c["implicit"].kind == "grid":
        out.append(("i64", CS.explicit(c["rows"], "cuda"), 0))
    return out


def _local(idx, offset):
    idx = np.asarray(idx)
    return np.where(idx >= 0, idx - offset, -1)


def run_topq(c, cands, offset, q=Q):
    """bo_select_topq over the shard with the per-call exclusion (the decode of every candidate that
    is probed against the evaluated points)."""
    import torch
    from bayesopt_smart_amd import _lib
    from bayesopt_smart_amd.acquisition import _grid_args
    lib = _lib.load()
    acq = torch.as_tensor(c["acq"], device="cuda")
    ex = torch.as_tensor(c["ev"], device="cuda")
    tv = torch.empty(q, dtype=torch.float64, device="cuda")
    ti = torch.empty(q, dtype=torch.int64, device="cuda")
    ws = torch.empty(lib.bo_select_topq_workspace_size(COUNT, q), dtype=torch.uint8, device="cuda")
    lo, sh = _grid_args(cands)
    carg = cands.tensor[offset:].data_ptr() if cands.kind in ("i64", "f64") else cands.cand_arg
    _lib.check(lib.bo_select_topq(acq.data_ptr(), COUNT, cands.kind_code, carg, lo, sh, cands.dim, offset,
                                  ex.data_ptr(), ex.shape[0], q, tv.data_ptr(), ti.data_ptr(), ws.data_ptr(),
                                  ws.numel(), None), "bo_select_topq")
    torch.cuda.synchronize()
    return {"top_idx": _local(ti.cpu().numpy(), offset), "top_val": tv.cpu().numpy()}


def run_mask(c, cands, offset):
    from bayesopt_smart_amd.acquisition import ExclusionMask
    m = ExclusionMask(cands, offset, COUNT, "cuda").update(c["ev"][:20]).update(c["ev"])
    return {"excluded": m.excluded()}


def run_bucb(c, cands, offset):
    import torch
    from bayesopt_smart_amd.acquisition import select_batch_bucb
    r = select_batch_bucb(torch.as_tensor(c["smu"], device="cuda"), torch.as_tensor(c["var"], device="cuda"), c["x"],
                          c["kinv"], cands, c["pv"], c["ls"], c["beta"], c["ev"], Q, offset=offset, count=COUNT,
                          return_details=True)
    out = {k: v.cpu().numpy() for k, v in r.items()}
    out["top_idx"] = _local(out["top_idx"], offset)
    return out


def run_paths(c, cands, offset):
    from bayesopt_smart_amd.acquisition import sample_paths
    paths, w = sample_paths(c["x"], c["y"], c["kinv"], cands, c["pm"], c["pv"], c["ls"], c["draws"], offset=offset,
                            count=COUNT, return_weights=True, device="cuda")
    return {"paths": paths.cpu().numpy(), "weights": w.cpu().numpy()}


def run_kb(c, cands, offset):
    import torch
    from bayesopt_smart_amd.acquisition import select_batch_kb
    r = select_batch_kb(torch.as_tensor(c["mu"], device="cuda"), torch.as_tensor(c["var"], device="cuda"), c["x"],
                        c["kinv"], cands, c["pv"], c["ls"], c["y"], N_TRAIN, c["y"].min(0) - 1.0, c["ev"], Q,
                        offset=offset, count=COUNT, return_details=True)
    out = {k: v.cpu().numpy() for k, v in r.items() if k != "n_boxes_max"}
    out["top_idx"] = _local(out["top_idx"], offset)
    return out


RUNNERS = {"topq": run_topq, "mask": run_mask, "bucb": run_bucb, "paths": run_paths, "kb": run_kb}

#!/usr/bin/env python
"""Time the hyper-parameter fit's two methods -- the native Powell fit and the L-BFGS-B fit over the
device's analytic MLL gradient (optimize_hyperparams_mll, method="lbfgs") -- on a config's bench
training set, in one process.

    python scripts/fit_lbfgs_bench.py --config C3 --out profiles/lbfgs_c3.jsonl [--loop]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \
        python scripts/fit_lbfgs_bench.py --config C3 --trace

The inputs are bench.py's (make_config_problem): x, y, pm, pv and the config's starting length scale.
Per method: the median wall time of --repeats fits from that start (and min .. max), nfev, the device
calls, the final MLL and length scales.  Then one bo_compute_mll_grad call against one
bo_compute_mll_each call (wall time, synchronous calls, median of --calls), and the L-BFGS fit's time
outside its device calls.  --loop adds the loop's timings["hyperparams"] with both methods from a
short BayesianOptimization run on the config's grid (grid configs only): the training set as the
initial design, 3 iterations of batch 3.  --trace runs three gradient calls and one fit of each
method only (for a kernel trace; no timing)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=("C2", "C3", "C4", "C5"), default="C3")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import bench
    from bayesopt_smart_amd import kernels as K

    cfg = bench.CONFIGS[args.config]
    x, y, pm, pv, ls, _, _, cand = bench.make_config_problem(cfg, 1)
    dev = torch.device("cuda", 0)
    n, n_obj = x.shape[0], len(pv)
    xd, yd = torch.as_tensor(x, device=dev), torch.as_tensor(y, device=dev)
    km = torch.zeros((n_obj, n, n), dtype=torch.float64, device=dev)

    def fit(method):
        lsv, pvv = ls.copy(), pv.copy()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        res = K.optimize_hyperparams_mll(xd, yd, km, pm, pvv, lsv, n, method=method)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, res, lsv

    def wall(fn, reps):
        out = []
        for _ in range(reps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            out.append((time.perf_counter() - t0) * 1e3)
        return out

    grad_call = lambda: K._mll_grad_call(xd, yd, km, pm, pv, ls, n, 1e-8)  # noqa: E731
    mll_call = lambda: K._mll_terms(xd, yd, km, pm, pv, ls, n, list(range(n_obj)), 1e-8)  # noqa: E731

    if args.trace:
        for _ in range(3):
            grad_call()
        for method in ("lbfgs", "powell"):
            fit(method)
        print(json.dumps({"trace": args.config}))
        return

    line = {"config": args.config, "n_train": int(n), "n_obj": n_obj, "dim": int(x.shape[1]), "ls0": float(ls[0]),
            "repeats": args.repeats, "device": torch.cuda.get_device_name(dev)}
    for method in ("powell", "lbfgs"):
        fit(method)                                            # warm-up (workspaces, pinned staging)
        runs = [fit(method) for _ in range(args.repeats)]
        ts = [r[0] for r in runs]
        _, res, lsv = runs[-1]
        line[method] = {"fit_ms": statistics.median(ts), "fit_spread_ms": [min(ts), max(ts)], "nfev": int(res.nfev),
                        "nit": int(res.nit), "device_calls": int(res.device_calls), "mll": float(-res.fun),
                        "ls": [float(v) for v in lsv], "message": str(res.message)}
    grad_call(), mll_call()
    g, m = wall(grad_call, args.calls), wall(mll_call, args.calls)
    line["mll_grad_call_ms"] = statistics.median(g)
    line["mll_grad_call_min_ms"] = min(g)
    line["mll_call_ms"] = statistics.median(m)
    line["mll_call_min_ms"] = min(m)
    # the same calls at the L-BFGS result (the fitted regime: longer length scales)
    ls_fit = np.array(line["lbfgs"]["ls"])
    gf = wall(lambda: K._mll_grad_call(xd, yd, km, pm, pv, ls_fit, n, 1e-8), args.calls)
    line["mll_grad_call_fitted_ms"] = statistics.median(gf)
    line["lbfgs_outside_device_calls_ms"] = line["lbfgs"]["fit_ms"] - line["lbfgs"]["device_calls"] * line["mll_grad_call_fitted_ms"]
    line["lbfgs_over_powell"] = line["lbfgs"]["fit_ms"] / line["powell"]["fit_ms"]
    line["mll_gap_over_ftol_margin"] = (line["powell"]["mll"] - line["lbfgs"]["mll"]) / (1e-4 * abs(line["powell"]["mll"]))

    if args.loop and cand[0] == "grid":
        from bayesopt_smart_amd import BayesianOptimization
        side = cand[2]
        for method in ("powell", "lbfgs"):
            hp = []
            opt = BayesianOptimization(bench._toy_point, [(0, side), (0, side)], n_objectives=n_obj, n_iterations=3,
                                       batch_size=3, initial_points=x, length_scales=ls.copy(), betas=[2.0] * n_obj,
                                       fit_method=method, callbacks=[lambda s: hp.append(s["timings"]["hyperparams"] * 1e3)])
            opt.optimize()
            line["loop_hyperparams_ms_" + method] = hp
    text = json.dumps(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Time the GIBBON batch (bo_select_batch_gibbon) beside its yardstick, bo_select_batch_bucb, in the
same process on the same posterior, and the whole "mes" select stage with batch_strategy "top" and
"gibbon".

    python scripts/gibbon_bench.py --config C3 --out profiles/gibbon_c3.jsonl
    python scripts/gibbon_bench.py --config C4 --out profiles/gibbon_c4.jsonl

The shapes are bench.py's C3 (1024 x 1024 grid, 2 objectives, N = 512) and C4 (2^21 Sobol points in
6-D, 3 objectives, N = 1024); the posterior is the predict's, computed once, and `base` is the
max-value entropy array of --samples posterior draws.

The cost of a FURTHER pick is (time of a call with q = --q-hi picks - time of a call with
q = --q-lo picks) / (q-hi - q-lo): HIP events around each device call, median of --calls calls per
block, the two strategies and the two batch sizes alternating inside every one of --alternations
blocks; the spread is min .. max over the blocks.  A further GIBBON pick does the update of a "bucb"
pick plus n_obj logs and (n_obj + 1) n_cand 8 bytes of extra reads (var^0 and base), so
`further_pick_ratio` = gibbon / bucb is the figure to watch: up to 1.10 is the extra reads and the
launch gap.  The stage lines are the wall time of acquisition.mes_select_indices (host work
included, synchronised) at each q of --stage-q.  One JSON line per measurement.
"""
import argparse
import ctypes
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
    ap.add_argument("--config", choices=["C3", "C4"], default="C3")
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--features", type=int, default=1024)
    ap.add_argument("--q-lo", type=int, default=2)
    ap.add_argument("--q-hi", type=int, default=10)
    ap.add_argument("--stage-q", type=int, nargs="+", default=[3, 16])
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5, help="timed calls per block")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import bench
    from bayesopt_smart_amd import _lib
    from bayesopt_smart_amd import acquisition as A
    from bayesopt_smart_amd.predict import CandidateSet, predict_acquire

    dev = torch.device("cuda", 0)
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    cfg = bench.CONFIGS[args.config]
    x, y, pm, pv, ls, betas, kinv, cand = bench.make_config_problem(cfg, 1)
    cands = CandidateSet.grid([(0, cand[1]), (0, cand[2])]) if cand[0] == "grid" else cand[1]
    n, m = cands.n, cfg["n_obj"]
    xd, yd, kd = (torch.as_tensor(a, device=dev) for a in (x, y, kinv))
    out = predict_acquire(xd, yd, kd, cands, pm, pv, ls, betas, outputs=("mu", "var", "std_mu"))
    mu, var, smu = out["mu"].contiguous(), out["var"].contiguous(), out["std_mu"].contiguous()
    mask = A.ExclusionMask(cands, 0, n, dev).update(x)
    draws = tuple(torch.as_tensor(a, device=dev) for a in
                  A.thompson_draws(np.random.default_rng(args.samples), m, cands.dim, x.shape[0], args.samples,
                                   args.features))
    base = torch.empty(n, dtype=torch.float64, device=dev)
    A.mes_select_indices(base, mu, var, xd, yd, kd, cands, pm, pv, ls, draws, x, 1, mask=mask, select=False)
    tv = torch.empty(_lib.MAX_TOPQ, dtype=torch.float64, device=dev)
    ti = torch.empty(_lib.MAX_TOPQ, dtype=torch.int64, device=dev)

    def fill(d, q):
        d.n_obj, d.n_train, d.q = m, x.shape[0], q
        d.x_train, d.kinv, d.ld_k = xd.data_ptr(), kd.data_ptr(), kd.shape[-1]
        A._set_cand_fields(d, cands, 0, n)
        for o in range(m):
            d.prior_var[o], d.length_scale[o] = float(pv[o]), float(ls[o])
        d.jitter, d.min_variance = 1e-6, 1e-10
        d.var, d.ld, d.mask = var.data_ptr(), n, mask.ptr
        d.top_val, d.top_idx = tv.data_ptr(), ti.data_ptr()
        return d

    def gibbon_call(q):
        d = fill(_lib.GibbonDesc(), q)
        d.base = base.data_ptr()
        ws = torch.empty(lib.bo_select_batch_gibbon_workspace_size(ctypes.byref(d)), dtype=torch.uint8, device=dev)
        return lambda: _lib.check(lib.bo_select_batch_gibbon(ctypes.byref(d), ws.data_ptr(), ws.numel(), stream),
                                  "bo_select_batch_gibbon")

    def bucb_call(q):
        d = fill(_lib.BucbDesc(), q)
        d.std_mu = smu.data_ptr()
        for o in range(m):
            d.beta[o] = float(betas[o])
        ws = torch.empty(lib.bo_select_batch_bucb_workspace_size(ctypes.byref(d)), dtype=torch.uint8, device=dev)
        return lambda: _lib.check(lib.bo_select_batch_bucb(ctypes.byref(d), ws.data_ptr(), ws.numel(), stream),
                                  "bo_select_batch_bucb")

    def timed(fn, k):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(k)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize(dev)
        return [a.elapsed_time(b) for a, b in ev]

    def wall(fn, k):
        ts = []
        for _ in range(k):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts

    common = {"config": args.config, "n_cand": n, "n_obj": m, "n_train": int(x.shape[0]), "n_samples": args.samples,
              "n_features": args.features, "alternations": args.alternations, "calls_per_block": args.calls,
              "device": torch.cuda.get_device_name(dev)}
    lines = []

    # ---- the cost of a further pick, gibbon beside bucb
    lo, hi = args.q_lo, args.q_hi
    calls = {"gibbon_lo": gibbon_call(lo), "bucb_lo": bucb_call(lo), "gibbon_hi": gibbon_call(hi),
             "bucb_hi": bucb_call(hi)}
    for fn in calls.values():
        fn()
    torch.cuda.synchronize(dev)
    med = {k: [] for k in calls}
    for _ in range(args.alternations):
        for name, fn in calls.items():
            timed(fn, 1)                                      # the block's own warm-up call
            med[name].append(statistics.median(timed(fn, args.calls)))
    per = {s: [(h - l) / (hi - lo) for h, l in zip(med[s + "_hi"], med[s + "_lo"])] for s in ("gibbon", "bucb")}
    ratio = [g / b for g, b in zip(per["gibbon"], per["bucb"])]
    line = dict(common, measure="further_pick", q_lo=lo, q_hi=hi,
                extra_read_bytes_per_pick=(m + 1) * n * 8, update_rows=int(x.shape[0]) + (lo + hi) // 2)
    for name, v in med.items():
        line[name + "_call_ms"] = statistics.median(v)
    for s in ("gibbon", "bucb"):
        line[s + "_further_pick_ms"] = statistics.median(per[s])
        line[s + "_further_pick_spread_ms"] = [min(per[s]), max(per[s])]
    line["further_pick_ratio"] = statistics.median(ratio)
    line["further_pick_ratio_spread"] = [min(ratio), max(ratio)]
    lines.append(line)
    print(json.dumps(line), flush=True)

    # ---- the whole "mes" select stage, "top" beside "gibbon"
    acq = torch.empty(n, dtype=torch.float64, device=dev)
    for q in args.stage_q:
        stages = {s: (lambda s=s: A.mes_select_indices(acq, mu, var, xd, yd, kd, cands, pm, pv, ls, draws, x, q,
                                                       mask=mask, batch_strategy=s)) for s in ("top", "gibbon")}
        picks = {s: np.asarray(fn()) for s, fn in stages.items()}
        med = {s: [] for s in stages}
        for _ in range(args.alternations):
            for s, fn in stages.items():
                wall(fn, 1)
                med[s].append(statistics.median(wall(fn, args.calls)))
        pts = cands.points(picks["gibbon"]).astype(np.float64), cands.points(picks["top"]).astype(np.float64)
        dist = [np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1))[np.triu_indices(len(p), 1)] for p in pts]
        line = dict(common, measure="mes_stage", q=q,
                    gibbon_min_pairwise_distance=float(dist[0].min()), top_max_pairwise_distance=float(dist[1].max()))
        for s, v in med.items():
            line[s + "_stage_wall_ms"] = statistics.median(v)
            line[s + "_stage_wall_spread_ms"] = [min(v), max(v)]
        line["gibbon_over_top"] = line["gibbon_stage_wall_ms"] / line["top_stage_wall_ms"]
        lines.append(line)
        print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(json.dumps(r) for r in lines) + "\n")


if __name__ == "__main__":
    main()

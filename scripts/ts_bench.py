#!/usr/bin/env python
"""Time the Thompson-sampling batch (bo_sample_paths, then the per-draw selection) against the
predict step and the hallucinated-observation batch (bo_select_batch_bucb) of the same shape, in one
process.

    python scripts/ts_bench.py --config C3 --out profiles/ts_c3.jsonl
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \
        python scripts/ts_bench.py --config C3 --trace

The shapes and seeded inputs are bench.py's (make_config_problem).  Each alternation times one block
per item with HIP events around every call: the fused predict + top-q as bench.py launches it; BUCB
at q = 3 and 16 on that predict's std_mu / var (unchanged code: what a diverse batch of q costs
without draws); for S = 1, 3, 16 and 48 draws the paths call (bo_sample_paths with D features: prep,
g(X), residual, mat-vec and the candidate pass) and, separately, the selection over the paths it
wrote ("sum_ucb": S times the sum over the objectives and the masked top-(s + 1)).  One JSON line per
alternation, then a summary line with the medians and the spread (min .. max of the alternations'
medians).  --trace runs a few calls only (for a kernel trace; no timing).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=("C3", "C4"), default="C3")
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10, help="timed calls per block")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--features", type=int, default=1024)
    ap.add_argument("--samples", type=int, nargs="*", default=[1, 3, 16, 48])
    ap.add_argument("--bucb-q", type=int, nargs="*", default=[3, 16])
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()

    import torch
    import bench
    from bayesopt_smart_amd import _lib
    from bayesopt_smart_amd.acquisition import ExclusionMask, thompson_draws
    from bayesopt_smart_amd.predict import CandidateSet, predict_acquire

    cfg = bench.CONFIGS[args.config]
    x, y, pm, pv, ls, betas, kinv, cand = bench.make_config_problem(cfg, 1)
    dev = torch.device("cuda", 0)
    cands = CandidateSet.grid([(0, cand[1]), (0, cand[2])]) if cand[0] == "grid" else cand[1]
    xd, yd, kd = (torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev) for a in (x, y, kinv))
    n_obj, m, n = len(pv), cands.n, x.shape[0]
    predict = predict_acquire(xd, yd, kd, cands, pm, pv, ls, betas, outputs=("std_mu", "var", "acq"),
                              topq=cfg["q"], device=dev, prepare=True)
    res = predict()
    mask = ExclusionMask(cands, 0, m, dev).update(x)
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream

    def shared(d):
        d.n_obj, d.dim, d.n_train = n_obj, cands.dim, n
        d.x_train, d.kinv, d.ld_k = xd.data_ptr(), kd.data_ptr(), n
        d.cand_kind, d.n_cand, d.cand_offset = cands.kind_code, m, 0
        if cands.kind == "grid":
            for k in range(cands.dim):
                d.grid_lo[k], d.grid_shape[k] = cands.lo[k], cands.shape[k]
        else:
            d.cand = cands.cand_arg
        for o in range(n_obj):
            d.prior_var[o], d.length_scale[o] = pv[o], ls[o]
        d.jitter = 1e-6

    def bucb_call(q):
        d = _lib.BucbDesc()
        shared(d)
        d.q = q
        for o in range(n_obj):
            d.beta[o] = betas[o]
        d.min_variance = 1e-10
        d.std_mu, d.var, d.ld = res["std_mu"].data_ptr(), res["var"].data_ptr(), res["var"].stride(0)
        d.mask = mask.ptr
        tv = torch.empty(q, dtype=torch.float64, device=dev)
        ti = torch.empty(q, dtype=torch.int64, device=dev)
        d.top_val, d.top_idx = tv.data_ptr(), ti.data_ptr()
        ws = torch.empty(lib.bo_select_batch_bucb_workspace_size(ctypes.byref(d)), dtype=torch.uint8, device=dev)

        def call():
            _lib.check(lib.bo_select_batch_bucb(ctypes.byref(d), ws.data_ptr(), ws.numel(), stream),
                       "bo_select_batch_bucb")
        call.keep = (d, tv, ti, ws)
        return call

    def ts_calls(n_s):
        draws = [torch.as_tensor(a, device=dev) for a in
                 thompson_draws(np.random.default_rng(0), n_obj, cands.dim, n, n_s, args.features)]
        d = _lib.TsDesc()
        shared(d)
        d.y, d.ld_y = yd.data_ptr(), yd.stride(0)
        d.n_samples, d.n_features = n_s, args.features
        for o in range(n_obj):
            d.prior_mean[o] = pm[o]
        d.z, d.phase, d.theta, d.eps = (t.data_ptr() for t in draws)
        paths = torch.empty((n_s, n_obj, m), dtype=torch.float64, device=dev)
        d.paths, d.ld = paths.data_ptr(), m
        ws = torch.empty(lib.bo_sample_paths_workspace_size(ctypes.byref(d)), dtype=torch.uint8, device=dev)
        acq = torch.empty(m, dtype=torch.float64, device=dev)
        rec = torch.empty(n_s * (n_s + 1), dtype=torch.float64, device=dev)
        sws = torch.empty(lib.bo_select_topq_workspace_size(m, n_s), dtype=torch.uint8, device=dev)

        def call_paths():
            _lib.check(lib.bo_sample_paths(ctypes.byref(d), ws.data_ptr(), ws.numel(), stream), "bo_sample_paths")

        def call_select():
            for s in range(n_s):
                tv = rec.data_ptr() + 8 * s * (s + 1)
                _lib.check(lib.bo_update_hypervolume_improvement(acq.data_ptr(), paths[s].data_ptr(), n_obj, m,
                                                                 stream), "bo_update_hypervolume_improvement")
                _lib.check(lib.bo_select_topq_masked(acq.data_ptr(), m, 0, mask.ptr, s + 1, tv, tv + 8 * (s + 1),
                                                     sws.data_ptr(), sws.numel(), stream), "bo_select_topq_masked")
        call_paths.keep = (d, draws, paths, ws, acq, rec, sws)
        return call_paths, call_select

    calls = {"predict_ms": predict}
    for q in args.bucb_q:
        calls[f"bucb_q{q}_ms"] = bucb_call(q)
    for n_s in args.samples:
        calls[f"ts_paths_s{n_s}_ms"], calls[f"ts_select_s{n_s}_ms"] = ts_calls(n_s)

    def timed(fn, k):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(k)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize(dev)
        return [a.elapsed_time(b) for a, b in ev]

    if args.trace:
        for fn in calls.values():
            timed(fn, 2)
        return
    for fn in calls.values():
        timed(fn, args.warmup)
    base = {"config": args.config, "n_train": int(n), "n_cand": int(m), "n_obj": n_obj, "dim": cands.dim,
            "features": args.features, "calls_per_block": args.calls, "device": torch.cuda.get_device_name(dev)}
    lines, med = [], {k: [] for k in calls}
    for alt in range(args.alternations):
        rec = dict(base, alternation=alt)
        for name, fn in calls.items():
            timed(fn, 1)                                      # the block's own warm-up call
            ts = timed(fn, args.calls)
            rec[name] = statistics.median(ts)
            rec[name.replace("_ms", "_min_ms")] = min(ts)
            med[name].append(rec[name])
        lines.append(rec)
    summary = dict(base, summary=True)
    for name, v in med.items():
        summary[name] = statistics.median(v)
        summary[name.replace("_ms", "_spread_ms")] = [min(v), max(v)]
    text = "\n".join(json.dumps(r) for r in lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()

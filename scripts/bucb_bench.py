#!/usr/bin/env python
"""Time the hallucinated-observation batch (bo_select_batch_bucb, q = 3) against the existing
predict step of the same shape, in one process.

    python scripts/bucb_bench.py --config C3 --out profiles/bucb_c3.jsonl
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \
        python scripts/bucb_bench.py --config C3 --trace

The shapes and seeded inputs are bench.py's (make_config_problem).  Each alternation times a block
of predict steps (the fused predict + top-q, as bench.py launches it), then a block of BUCB calls
on that predict's std_mu / var (q = 3 and q = 1, without var_out: what the loop runs), with HIP
events around every call; one JSON line per alternation, then a summary line with the medians and
the spread (min .. max of the alternations' medians).  A step of the batch is (q3 - q1) / 2: one
pick, one mat-vec, one coefficient kernel and one candidate pass.  --trace runs a few calls only
(for a kernel trace; no timing).
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
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--q", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()

    import torch
    import bench
    from bayesopt_smart_amd import _lib
    from bayesopt_smart_amd.acquisition import ExclusionMask
    from bayesopt_smart_amd.predict import CandidateSet, predict_acquire

    cfg = bench.CONFIGS[args.config]
    x, y, pm, pv, ls, betas, kinv, cand = bench.make_config_problem(cfg, 1)
    dev = torch.device("cuda", 0)
    cands = CandidateSet.grid([(0, cand[1]), (0, cand[2])]) if cand[0] == "grid" else cand[1]
    xd, yd, kd = (torch.as_tensor(a, device=dev) for a in (x, y, kinv))
    n_obj, m = len(pv), cands.n
    predict = predict_acquire(xd, yd, kd, cands, pm, pv, ls, betas, outputs=("std_mu", "var", "acq"),
                              topq=cfg["q"], device=dev, prepare=True)
    res = predict()
    mask = ExclusionMask(cands, 0, m, dev).update(x)
    lib = _lib.load()

    def bucb_call(q):
        d = _lib.BucbDesc()
        d.n_obj, d.dim, d.n_train = n_obj, cands.dim, x.shape[0]
        d.x_train, d.kinv, d.ld_k = xd.data_ptr(), kd.data_ptr(), x.shape[0]
        d.cand_kind, d.q, d.n_cand, d.cand_offset = cands.kind_code, q, m, 0
        if cands.kind == "grid":
            for k in range(cands.dim):
                d.grid_lo[k], d.grid_shape[k] = cands.lo[k], cands.shape[k]
        else:
            d.cand = cands.cand_arg
        for o in range(n_obj):
            d.prior_var[o], d.length_scale[o], d.beta[o] = pv[o], ls[o], betas[o]
        d.jitter, d.min_variance = 1e-6, 1e-10
        d.std_mu, d.var, d.ld = res["std_mu"].data_ptr(), res["var"].data_ptr(), res["var"].stride(0)
        d.mask = mask.ptr
        tv = torch.empty(q, dtype=torch.float64, device=dev)
        ti = torch.empty(q, dtype=torch.int64, device=dev)
        d.top_val, d.top_idx = tv.data_ptr(), ti.data_ptr()
        ws = torch.empty(lib.bo_select_batch_bucb_workspace_size(ctypes.byref(d)), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream

        def call():
            _lib.check(lib.bo_select_batch_bucb(ctypes.byref(d), ws.data_ptr(), ws.numel(), stream),
                       "bo_select_batch_bucb")
        call.keep = (d, tv, ti, ws)
        return call

    calls = {"predict_ms": predict, f"bucb_q{args.q}_ms": bucb_call(args.q), "bucb_q1_ms": bucb_call(1)}

    def timed(fn, n):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize(dev)
        return [a.elapsed_time(b) for a, b in ev]

    if args.trace:
        for fn in calls.values():
            timed(fn, 3)
        return
    for fn in calls.values():
        timed(fn, args.warmup)
    base = {"config": args.config, "n_train": int(x.shape[0]), "n_cand": int(m), "n_obj": n_obj, "dim": cands.dim,
            "q": args.q, "calls_per_block": args.calls, "device": torch.cuda.get_device_name(dev)}
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
    q3, q1, p = (summary[f"bucb_q{args.q}_ms"], summary["bucb_q1_ms"], summary["predict_ms"])
    summary["bucb_step_ms"] = (q3 - q1) / max(args.q - 1, 1)
    summary["bucb_over_predict"] = q3 / p
    summary["step_over_predict"] = summary["bucb_step_ms"] / p
    lines.append(summary)
    text = "\n".join(json.dumps(r) for r in lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()

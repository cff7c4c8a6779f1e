#!/usr/bin/env python
"""Time the Kriging-believer batch for the EHVI (bo_select_batch_kb) at q = 1, 3 and 16 against the
predict step, the hallucinated-observation batch (bo_select_batch_bucb) at the same q, and the plain
EHVI scan plus its masked selection, all at one shape and in one process.

    python scripts/kb_bench.py --config C3 --out profiles/kb_c3.jsonl
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \
        python scripts/kb_bench.py --config C3 --trace 16

The shapes and seeded inputs are bench.py's (make_config_problem); the front is 16 mutually
non-dominated points around the prior mean (on a sphere of 1.5 prior standard deviations), the
reference point two standard deviations below it.  Each alternation times a block of calls of every
kind with HIP events around every call; one JSON line per alternation, then a summary line with the
medians and the spread (min .. max of the alternations' medians).  The believer's call waits on the
host once per pick, so its events bracket the host steps as well: `kb_q*_ms` is the call as the
stream sees it, `kb_q*_wall_ms` the host's time from the call to the end of the stream's work.  A
further pick costs (q16 - q1) / 15.  --trace Q runs three calls of the believer at q = Q only (for a
kernel trace, whose summed kernel time against the wall time shows what the host adds; no timing).
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

QS = (1, 3, 16)


def make_front(rng, m, p):
    """p mutually non-dominated points: on the positive part of a sphere of radius 1.5."""
    v = np.abs(rng.normal(size=(p, m))) + 0.05
    return 1.5 * v / np.linalg.norm(v, axis=1, keepdims=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=("C3", "C4"), default="C3")
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10, help="timed calls per block")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--front", type=int, default=16)
    ap.add_argument("--box-capacity", type=int, default=4096)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", type=int, default=0, metavar="Q")
    args = ap.parse_args()

    import torch
    import bench
    from bayesopt_smart_amd import _lib
    from bayesopt_smart_amd.acquisition import EhviTables, ExclusionMask
    from bayesopt_smart_amd.predict import CandidateSet, predict_acquire

    cfg = bench.CONFIGS[args.config]
    x, y, pm, pv, ls, betas, kinv, cand = bench.make_config_problem(cfg, 1)
    dev = torch.device("cuda", 0)
    cands = CandidateSet.grid([(0, cand[1]), (0, cand[2])]) if cand[0] == "grid" else cand[1]
    xd, yd, kd = (torch.as_tensor(a, device=dev) for a in (x, y, kinv))
    n_obj, m = len(pv), cands.n
    predict = predict_acquire(xd, yd, kd, cands, pm, pv, ls, betas, outputs=("mu", "std_mu", "var", "acq"),
                              topq=cfg["q"], device=dev, prepare=True)
    res = predict()
    mask = ExclusionMask(cands, 0, m, dev).update(x)
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    rng = np.random.default_rng(7)
    sd = np.sqrt(np.asarray(pv, dtype=np.float64))
    front = np.ascontiguousarray(np.asarray(pm) + sd * make_front(rng, n_obj, args.front))
    ref = np.asarray(pm) - 2.0 * sd

    def common(d):
        d.n_obj, d.dim, d.n_train = n_obj, cands.dim, x.shape[0]
        d.x_train, d.kinv, d.ld_k = xd.data_ptr(), kd.data_ptr(), x.shape[0]
        d.cand_kind, d.n_cand, d.cand_offset = cands.kind_code, m, 0
        if cands.kind == "grid":
            for k in range(cands.dim):
                d.grid_lo[k], d.grid_shape[k] = cands.lo[k], cands.shape[k]
        else:
            d.cand = cands.cand_arg
        for o in range(n_obj):
            d.prior_var[o], d.length_scale[o] = pv[o], ls[o]
        d.jitter, d.min_variance = 1e-6, 1e-10
        d.var, d.ld, d.mask = res["var"].data_ptr(), res["var"].stride(0), mask.ptr

    def bucb_call(q):
        d = _lib.BucbDesc()
        common(d)
        d.q = q
        for o in range(n_obj):
            d.beta[o] = betas[o]
        d.std_mu = res["std_mu"].data_ptr()
        tv = torch.empty(q, dtype=torch.float64, device=dev)
        ti = torch.empty(q, dtype=torch.int64, device=dev)
        d.top_val, d.top_idx = tv.data_ptr(), ti.data_ptr()
        ws = torch.empty(lib.bo_select_batch_bucb_workspace_size(ctypes.byref(d)), dtype=torch.uint8, device=dev)

        def call():
            _lib.check(lib.bo_select_batch_bucb(ctypes.byref(d), ws.data_ptr(), ws.numel(), stream),
                       "bo_select_batch_bucb")
        call.keep = (d, tv, ti, ws)
        return call

    def kb_call(q):
        d = _lib.KbDesc()
        common(d)
        d.q = q
        d.mu = res["mu"].data_ptr()
        d.front, d.n_front = front.ctypes.data, front.shape[0]
        for o in range(n_obj):
            d.ref_point[o] = ref[o]
        d.form, d.box_capacity = 0, args.box_capacity
        tv = torch.empty(q, dtype=torch.float64, device=dev)
        ti = torch.empty(q, dtype=torch.int64, device=dev)
        bl = torch.empty((q, n_obj), dtype=torch.float64, device=dev)
        d.top_val, d.top_idx, d.believed = tv.data_ptr(), ti.data_ptr(), bl.data_ptr()
        met = ctypes.c_int64(0)
        d.n_boxes_max = ctypes.pointer(met)
        ws = torch.empty(lib.bo_select_batch_kb_workspace_size(ctypes.byref(d)), dtype=torch.uint8, device=dev)
        hws = torch.empty(lib.bo_select_batch_kb_host_workspace_size(ctypes.byref(d)), dtype=torch.uint8).pin_memory()
        d.host_ws, d.host_ws_bytes = hws.data_ptr(), hws.numel()

        def call():
            _lib.check(lib.bo_select_batch_kb(ctypes.byref(d), ws.data_ptr(), ws.numel(), stream),
                       "bo_select_batch_kb")
        call.keep = (d, tv, ti, bl, ws, hws)
        call.met = met
        call.picks = ti
        return call

    tb = EhviTables(front, ref, dev)
    acq = torch.empty(m, dtype=torch.float64, device=dev)
    rec = torch.empty(2 * 3, dtype=torch.float64, device=dev)
    sel_ws = torch.empty(lib.bo_select_topq_workspace_size(m, 3), dtype=torch.uint8, device=dev)

    def ehvi_select():
        _lib.check(lib.bo_expected_hypervolume_improvement(
            acq.data_ptr(), res["mu"].data_ptr(), res["var"].data_ptr(), res["var"].stride(0), m, n_obj,
            tb.boxes.data_ptr(), tb.n_boxes, tb.edges.data_ptr(), tb.n_edges, tb.box_idx.data_ptr(), 0, stream),
            "bo_expected_hypervolume_improvement")
        _lib.check(lib.bo_select_topq_masked(acq.data_ptr(), m, 0, mask.ptr, 3, rec.data_ptr(), rec.data_ptr() + 24,
                                             sel_ws.data_ptr(), sel_ws.numel(), stream), "bo_select_topq_masked")

    def timed(fn, n):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize(dev)
        return [a.elapsed_time(b) for a, b in ev]

    def wall(fn, n):
        out = []
        for _ in range(n):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            out.append((time.perf_counter() - t0) * 1e3)
        return out

    if args.trace:
        fn = kb_call(args.trace)
        timed(fn, 1)
        print(json.dumps({"trace_q": args.trace, "kb_wall_ms": wall(fn, 3), "n_boxes_max": fn.met.value}))
        return
    kb = {q: kb_call(q) for q in QS}
    calls = {"predict_ms": predict, "ehvi_select_q3_ms": ehvi_select}
    for q in QS:
        calls[f"bucb_q{q}_ms"] = bucb_call(q)
        calls[f"kb_q{q}_ms"] = kb[q]
    for fn in calls.values():
        timed(fn, args.warmup)
    base = {"config": args.config, "n_train": int(x.shape[0]), "n_cand": int(m), "n_obj": n_obj, "dim": cands.dim,
            "front": int(front.shape[0]), "n_boxes_first": int(tb.n_boxes), "sum_edges_first": int(tb.sum_edges),
            "n_boxes_max": {str(q): int(kb[q].met.value) for q in QS},
            "distinct_picks_q16": int(len(set(kb[16].picks.cpu().numpy().tolist()))),
            "calls_per_block": args.calls, "device": torch.cuda.get_device_name(dev)}
    lines, med = [], {}
    for alt in range(args.alternations):
        r = dict(base, alternation=alt)
        for name, fn in calls.items():
            timed(fn, 1)                                      # the block's own warm-up call
            ts = timed(fn, args.calls)
            r[name] = statistics.median(ts)
            r[name.replace("_ms", "_min_ms")] = min(ts)
            med.setdefault(name, []).append(r[name])
            if name.startswith("kb_"):
                w = name.replace("_ms", "_wall_ms")
                r[w] = statistics.median(wall(fn, args.calls))
                med.setdefault(w, []).append(r[w])
        lines.append(r)
    summary = dict(base, summary=True)
    for name, v in med.items():
        summary[name] = statistics.median(v)
        summary[name.replace("_ms", "_spread_ms")] = [min(v), max(v)]
    summary["kb_step_ms"] = (summary["kb_q16_ms"] - summary["kb_q1_ms"]) / 15.0
    summary["bucb_step_ms"] = (summary["bucb_q16_ms"] - summary["bucb_q1_ms"]) / 15.0
    summary["kb_q3_over_predict"] = summary["kb_q3_ms"] / summary["predict_ms"]
    lines.append(summary)
    text = "\n".join(json.dumps(r) for r in lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()

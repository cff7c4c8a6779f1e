#!/usr/bin/env python
"""Time the "mes" select stage -- bo_sample_paths, bo_path_maxima, bo_max_value_entropy, the masked
top-q -- per kernel and as a whole, beside the "ehvi" select stage at the same shape in the same
process for scale.

    python scripts/mes_bench.py --config C3 --out profiles/mes_c3.jsonl
    python scripts/mes_bench.py --config C4 --out profiles/mes_c4.jsonl

The shapes are bench.py's C3 (1024 x 1024 grid, 2 objectives, N = 512) and C4 (2^21 Sobol points in
6-D, 3 objectives, N = 1024); the posterior is the predict's, computed once.  Per S in --samples:
HIP events around each device call (median of --calls calls per block, --alternations blocks; the
spread is min .. max of the blocks' medians), and the wall time of the whole stage
(acquisition.mes_select_indices / ehvi_select_indices, host work included, synchronised).  One JSON
line per S.

Kernel durations without the events' launch gaps: a traced run of its own with one S, then its summary
appended to the same file,

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \
        python scripts/mes_bench.py --config C3 --samples 16 --alternations 2
    python scripts/mes_bench.py --config C3 --samples 16 --trace DIR/.../run_kernel_trace.csv --out profiles/mes_c3.jsonl
"""
import argparse
import json
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summarize_trace(args):
    """Median duration per kernel of a `rocprofv3 --kernel-trace --stats --output-format csv` run of this
    script: the stage's own kernels (the draws, the maxima, the scan, the selection, the EHVI scan)."""
    import csv
    dur = {}
    with open(args.trace, newline="") as fh:
        for row in csv.DictReader(fh):
            full = row["Kernel_Name"].replace("(anonymous namespace)::", "")
            m = re.search(r"([A-Za-z_][A-Za-z_0-9]*)(<[^()]*>)?\s*\(", full)
            name = (m.group(1) + (m.group(2) or "")) if m else full
            dur.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3)
    keep = ("ts_", "path_maxima", "mes_scan", "select_", "ehvi_", "merge")
    line = {"config": args.config, "n_samples": args.samples[0], "source": "rocprofv3 --kernel-trace",
            "kernel_median_us": {k: statistics.median(v) for k, v in sorted(dur.items()) if any(s in k for s in keep)},
            "kernel_calls": {k: len(v) for k, v in sorted(dur.items()) if any(s in k for s in keep)}}
    print(json.dumps(line))
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=["C3", "C4"], default="C3")
    ap.add_argument("--samples", type=int, nargs="+", default=[4, 8, 16])
    ap.add_argument("--features", type=int, default=1024)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5, help="timed calls per block")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", default=None, help="summarise this rocprofv3 kernel-trace CSV (of a run of this "
                    "script with one --samples value) and append the line to --out; runs nothing")
    args = ap.parse_args()
    if args.trace:
        return summarize_trace(args)

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
    n, m, q = cands.n, cfg["n_obj"], cfg["q"]
    xd, yd, kd = (torch.as_tensor(a, device=dev) for a in (x, y, kinv))
    out = predict_acquire(xd, yd, kd, cands, pm, pv, ls, betas, outputs=("mu", "var"))
    mu, var = out["mu"].contiguous(), out["var"].contiguous()
    acq = torch.empty(n, dtype=torch.float64, device=dev)
    mask = A.ExclusionMask(cands, 0, n, dev).update(x)
    ref_point = y.min(axis=0) - 1.0
    rec = torch.empty(2 * q, dtype=torch.float64, device=dev)
    ws_sel = torch.empty(lib.bo_select_topq_workspace_size(n, q), dtype=torch.uint8, device=dev)

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

    def select():
        _lib.check(lib.bo_select_topq_masked(acq.data_ptr(), n, 0, mask.ptr, q, rec.data_ptr(),
                                             rec.data_ptr() + 8 * q, ws_sel.data_ptr(), ws_sel.numel(), stream),
                   "bo_select_topq_masked")

    tables = A.EhviTables(A._front_of(y, len(y), ref_point), ref_point, dev)

    def ehvi_scan():
        A.expected_hypervolume_improvement(mu, var, None, None, out=acq, tables=tables)

    def ehvi_stage():
        A.ehvi_select_indices(acq, mu, var, y, len(y), ref_point, cands, x, q, return_record=True, mask=mask)

    lines = []
    for n_s in args.samples:
        draws = tuple(torch.as_tensor(a, device=dev) for a in
                      A.thompson_draws(np.random.default_rng(n_s), m, cands.dim, x.shape[0], n_s, args.features))
        paths = A.sample_paths(xd, yd, kd, cands, pm, pv, ls, draws, device=dev)
        ystar = A.path_maxima(paths, pm, pv)
        ws_max = torch.empty(lib.bo_path_maxima_workspace_size(n, n_s * m), dtype=torch.uint8, device=dev)
        shift, scale = _lib.dbl_array(pm, m), _lib.dbl_array(np.sqrt(pv), m)

        def gen():
            A.sample_paths(xd, yd, kd, cands, pm, pv, ls, draws, device=dev)

        def maxima():
            _lib.check(lib.bo_path_maxima(ystar.data_ptr(), paths.data_ptr(), n, n, n_s, m, shift, scale,
                                          ws_max.data_ptr(), ws_max.numel(), stream), "bo_path_maxima")

        def scan():
            _lib.check(lib.bo_max_value_entropy(acq.data_ptr(), mu.data_ptr(), var.data_ptr(), n, n, m,
                                                ystar.data_ptr(), n_s, stream), "bo_max_value_entropy")

        def mes_stage():
            A.mes_select_indices(acq, mu, var, xd, yd, kd, cands, pm, pv, ls, draws, x, q, return_record=True,
                                 mask=mask)

        calls = {"sample_paths_ms": gen, "path_maxima_ms": maxima, "mes_scan_ms": scan, "select_ms": select,
                 "ehvi_scan_ms": ehvi_scan}
        stages = {"mes_stage_wall_ms": mes_stage, "ehvi_stage_wall_ms": ehvi_stage}
        for fn in list(calls.values()) + list(stages.values()):
            fn()
        torch.cuda.synchronize(dev)
        med = {k: [] for k in list(calls) + list(stages)}
        for _ in range(args.alternations):
            for name, fn in calls.items():
                timed(fn, 1)                                      # the block's own warm-up call
                med[name].append(statistics.median(timed(fn, args.calls)))
            for name, fn in stages.items():
                wall(fn, 1)
                med[name].append(statistics.median(wall(fn, args.calls)))
        line = {"config": args.config, "n_cand": n, "n_obj": m, "n_train": int(x.shape[0]), "n_samples": n_s,
                "n_features": args.features, "q": q, "n_boxes": tables.n_boxes, "paths_bytes": n_s * m * n * 8,
                "g_evaluations": n_s * m * n, "alternations": args.alternations, "calls_per_block": args.calls,
                "device": torch.cuda.get_device_name(dev)}
        for name, v in med.items():
            line[name] = statistics.median(v)
            line[name.replace("_ms", "_spread_ms")] = [min(v), max(v)]
        line["path_maxima_gb_per_s"] = line["paths_bytes"] / (line["path_maxima_ms"] * 1e-3) / 1e9
        line["g_per_s"] = line["g_evaluations"] / (line["mes_scan_ms"] * 1e-3)
        line["mes_scan_over_ehvi_scan"] = line["mes_scan_ms"] / line["ehvi_scan_ms"]
        lines.append(line)
        print(json.dumps(line), flush=True)
        del paths, draws
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(json.dumps(r) for r in lines) + "\n")


if __name__ == "__main__":
    main()

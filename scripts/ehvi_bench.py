#!/usr/bin/env python
"""Time the EHVI scan (bo_expected_hypervolume_improvement) in its table form and its direct form,
and the existing fused exact-HVI scan + top-q (bo_hvi_select_topq_masked) at the same shape as
context, in one process.

    python scripts/ehvi_bench.py --out profiles/ehvi_c3.jsonl

Shapes, all at 2^20 candidates: 2 objectives with fronts of 8, 16 and 32 points (the C3 shape: a
1024 x 1024 grid, 2 objectives) and 3 objectives with fronts of 16 and 32 points, then the shapes
that bracket auto's rule (SHAPES below).  The fronts are
mutually non-dominated points with distinct coordinates (every point adds an edge on every axis),
mu / var seeded random posteriors around them.  Each alternation times a block of table calls,
a block of direct calls and a block of HVI calls, with HIP events around every call; one JSON line
per shape with the median and the spread (min .. max) of the alternations' medians, the boxes, the
edges, the psi evaluations per call of each form and the psi evaluations per second reached.
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

# the issue's five shapes, then what brackets auto's rule: 2 objectives at the last sum of edges with
# two 256-thread tables per CU (40) and the first with one (42); 3 objectives down to a 64-thread
# table with one wave per CU; 4 objectives
SHAPES = ((2, 8), (2, 16), (2, 32), (3, 16), (3, 32), (2, 19), (2, 20), (3, 64), (3, 100), (4, 8), (4, 16))


def make_front(rng, m, p):
    """p mutually non-dominated points: on the positive part of a sphere of radius 4."""
    v = np.abs(rng.normal(size=(p, m))) + 0.05
    return 4.0 * v / np.linalg.norm(v, axis=1, keepdims=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5, help="timed calls per block")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from bayesopt_smart_amd import _lib
    from bayesopt_smart_amd.acquisition import EhviTables

    dev = torch.device("cuda", 0)
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    n = args.n

    def timed(fn, k):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(k)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize(dev)
        return [a.elapsed_time(b) for a, b in ev]

    lines = []
    for m, p in SHAPES:
        rng = np.random.default_rng(100 * m + p)
        front = make_front(rng, m, p)
        ref = np.zeros(m)
        tb = EhviTables(front, ref, dev)
        boxes = tb.boxes.cpu().numpy()
        mu = torch.as_tensor(rng.normal(size=(m, n)) * 1.5 + 2.0, device=dev)
        var = torch.as_tensor(rng.uniform(0.01, 2.0, size=(m, n)), device=dev)
        ucb = mu + 2.0 * var.sqrt()
        acq = torch.empty(n, dtype=torch.float64, device=dev)
        mask = torch.zeros(lib.bo_excl_mask_bytes(n) // 4, dtype=torch.int32, device=dev)
        q = 3
        rec = torch.empty(2 * q, dtype=torch.float64, device=dev)
        ws = torch.empty(lib.bo_select_topq_workspace_size(n, q), dtype=torch.uint8, device=dev)
        shift, scale = (ctypes.c_double * m)(*([0.0] * m)), (ctypes.c_double * m)(*([1.0] * m))

        def ehvi(form):
            def call():
                _lib.check(lib.bo_expected_hypervolume_improvement(
                    acq.data_ptr(), mu.data_ptr(), var.data_ptr(), n, n, m, tb.boxes.data_ptr(), tb.n_boxes,
                    tb.edges.data_ptr(), tb.n_edges, tb.box_idx.data_ptr(), form, stream),
                    "bo_expected_hypervolume_improvement")
            return call

        def hvi():
            _lib.check(lib.bo_hvi_select_topq_masked(acq.data_ptr(), ucb.data_ptr(), n, n, m, shift, scale,
                                                     tb.boxes.data_ptr(), tb.n_boxes, 0, mask.data_ptr(), q,
                                                     rec.data_ptr(), rec.data_ptr() + 8 * q, ws.data_ptr(),
                                                     ws.numel(), stream), "bo_hvi_select_topq_masked")

        calls = {"hvi_select_ms": hvi, "direct_ms": ehvi(1)}
        if tb.threads:
            calls["table_ms"] = ehvi(2)
        for fn in calls.values():
            timed(fn, args.warmup)
        med = {k: [] for k in calls}
        for _ in range(args.alternations):
            for name, fn in calls.items():
                timed(fn, 1)                                      # the block's own warm-up call
                med[name].append(statistics.median(timed(fn, args.calls)))
        psi_direct = int(np.isfinite(boxes).sum())               # +inf bounds are skipped
        rec_line = {"n_cand": n, "n_obj": m, "front": p, "n_boxes": tb.n_boxes,
                    "n_edges": [int(e) for e in tb.n_edges], "sum_edges": tb.sum_edges,
                    "table_threads": tb.threads, "psi_per_cand_direct": psi_direct,
                    "psi_per_cand_table": tb.sum_edges, "alternations": args.alternations,
                    "calls_per_block": args.calls, "device": torch.cuda.get_device_name(dev)}
        for name, v in med.items():
            rec_line[name] = statistics.median(v)
            rec_line[name.replace("_ms", "_spread_ms")] = [min(v), max(v)]
        rec_line["direct_psi_per_s"] = psi_direct * n / (rec_line["direct_ms"] * 1e-3)
        if tb.threads:
            rec_line["table_psi_per_s"] = tb.sum_edges * n / (rec_line["table_ms"] * 1e-3)
            rec_line["direct_over_table"] = rec_line["direct_ms"] / rec_line["table_ms"]
            rec_line["table_not_slower"] = max(med["table_ms"]) <= min(med["direct_ms"])
        lines.append(rec_line)
        print(json.dumps(rec_line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(json.dumps(r) for r in lines) + "\n")


if __name__ == "__main__":
    main()

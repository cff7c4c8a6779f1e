#!/usr/bin/env python
"""Time the constrained EHVI scan (bo_constrained_ehvi) against the plain scan of the same build
(bo_expected_hypervolume_improvement) and against the unfused composition -- the plain scan, then
the probability of feasibility and the product as torch operations -- in one process.

    python scripts/cehvi_bench.py --out profiles/cehvi_c3.jsonl

Shapes, all at 2^20 candidates: 2 objectives and 3 objectives with a 16-point front
(scripts/ehvi_bench.py's fronts and posteriors), each with 1, 2 and 4 constraints whose bounds
rotate through two-sided, one-sided each way and narrow.  The form is auto's.  Each alternation
times a block of constrained calls, a block of plain calls and a block of composed calls, with HIP
events around every call; one JSON line per shape with the median and the spread (min .. max) of
the alternations' medians.  The composition evaluates the same formula (the difference of positive
tail terms, torch.special.erfc) and is checked against the scan before it is timed.
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

SHAPES = tuple((m, 16, c) for m in (2, 3) for c in (1, 2, 4))
KINDS = ((-0.5, 1.5), (-np.inf, 1.0), (0.0, np.inf), (0.3, 0.4))


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
    for m, p, c in SHAPES:
        rng = np.random.default_rng(100 * m + p)
        front = make_front(rng, m, p)
        tb = EhviTables(front, np.zeros(m), dev)
        mu = torch.as_tensor(np.vstack([rng.normal(size=(m, n)) * 1.5 + 2.0, rng.normal(size=(c, n))]), device=dev)
        var = torch.as_tensor(np.vstack([rng.uniform(0.01, 2.0, size=(m, n)), rng.uniform(0.05, 2.0, size=(c, n))]),
                              device=dev)
        bounds = [KINDS[j % 4] for j in range(c)]
        lo = (ctypes.c_double * c)(*[b[0] for b in bounds])
        hi = (ctypes.c_double * c)(*[b[1] for b in bounds])
        acq = torch.empty(n, dtype=torch.float64, device=dev)
        pof = torch.empty(n, dtype=torch.float64, device=dev)
        acq2 = torch.empty(n, dtype=torch.float64, device=dev)
        tabs = (tb.boxes.data_ptr(), tb.n_boxes, tb.edges.data_ptr(), tb.n_edges, tb.box_idx.data_ptr(), 0, stream)

        def constrained():
            _lib.check(lib.bo_constrained_ehvi(acq.data_ptr(), pof.data_ptr(), mu.data_ptr(), var.data_ptr(), n, n,
                                               m, c, lo, hi, *tabs), "bo_constrained_ehvi")

        def plain():
            _lib.check(lib.bo_expected_hypervolume_improvement(acq2.data_ptr(), mu.data_ptr(), var.data_ptr(), n, n,
                                                               m, *tabs), "bo_expected_hypervolume_improvement")

        def tail(z):
            return 0.5 * torch.special.erfc(z * 0.7071067811865476)

        def composed():
            plain()
            prod = None
            for j, (a, b) in enumerate(bounds):
                sg = var[m + j].abs().sqrt()
                za, zb = (a - mu[m + j]) / sg, (b - mu[m + j]) / sg
                above = za > 0
                below = ~above & (zb < 0)
                q1 = tail(torch.where(above, za, torch.where(below, -zb, zb)))
                q2 = tail(torch.where(above, zb, -za))
                pj = torch.where(above | below, q1, 1.0 - q1) - q2
                prod = pj if prod is None else prod * pj
            acq2.mul_(prod)

        constrained()
        composed()
        torch.cuda.synchronize(dev)
        rel = ((acq - acq2).abs() / acq.abs().clamp_min(1e-300)).max().item()
        if not rel < 1e-6:
            raise SystemExit(f"the composition differs from the scan: rel {rel}")
        calls = {"constrained_ms": constrained, "plain_ms": plain, "composed_ms": composed}
        for fn in calls.values():
            timed(fn, args.warmup)
        med = {k: [] for k in calls}
        for _ in range(args.alternations):
            for name, fn in calls.items():
                timed(fn, 1)                                      # the block's own warm-up call
                med[name].append(statistics.median(timed(fn, args.calls)))
        rec_line = {"n_cand": n, "n_obj": m, "n_con": c, "front": p, "n_boxes": tb.n_boxes,
                    "sum_edges": tb.sum_edges, "table_threads": tb.threads, "form": "auto",
                    "bounds": [[str(a), str(b)] for a, b in bounds], "alternations": args.alternations,
                    "calls_per_block": args.calls, "composition_max_rel_diff": rel,
                    "device": torch.cuda.get_device_name(dev)}
        for name, v in med.items():
            rec_line[name] = statistics.median(v)
            rec_line[name.replace("_ms", "_spread_ms")] = [min(v), max(v)]
        rec_line["constrained_over_plain"] = rec_line["constrained_ms"] / rec_line["plain_ms"]
        rec_line["composed_over_constrained"] = rec_line["composed_ms"] / rec_line["constrained_ms"]
        # slower than the composition beyond the alternations' spread: every block slower than every block
        rec_line["fused_slower_than_composition"] = min(med["constrained_ms"]) > max(med["composed_ms"])
        lines.append(rec_line)
        print(json.dumps(rec_line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(json.dumps(r) for r in lines) + "\n")


if __name__ == "__main__":
    main()

"""Time the grid-convolution path per width of the contraction's wave tile: graph-replayed "auto-conv" calls
(2 objectives, q = 3, the selection alone; gridconv_crossover.py's problems and timing) with BO_CONV_TILE unset
(the plan's choice) and forced to 1, 2 and 4, microseconds per call.  The library is the one BO_AMD_LIB names;
a library without the knob is measured with TILES=auto.

    [TILES=auto,1,2,4] python scripts/gridconv_tile_sweep.py [big]     # one JSON line per shape
Without `big`: sides 64 / 256 / 512 / 1024 x N = 32 .. 512 (profiles/ctile_tile_sweep.jsonl, first part);
with it: the grids above 2^20 candidates of its second part, each setting timed twice."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gridconv_crossover as X  # noqa: E402
import bayesopt_smart_amd as bo  # noqa: E402


def time_us(d, rows, side):
    cands = bo.predict.CandidateSet.grid([(0, rows), (0, side)])
    prepared = bo.predict.predict_acquire(d["x"], d["y"], d["Kinv"], cands, d["pm"], d["pv"], d["ls"], d["betas"],
                                          outputs=(), topq=3, mode="auto-conv", prepare=True)
    replay = prepared.graphed()
    for _ in range(5):
        replay()
    torch.cuda.synchronize()
    best = None
    for _ in range(3):                       # the best of three rounds of REPS back-to-back replays
        t0 = time.perf_counter()
        for _ in range(X.REPS):
            replay()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / X.REPS * 1e6
        best = dt if best is None else min(best, dt)
    return best, prepared.res["top_idx"].cpu().numpy().tolist()


def main():
    big = len(sys.argv) > 1 and sys.argv[1] == "big"
    lib = os.path.basename(os.environ.get("BO_AMD_LIB", "libbo_amd.so"))
    tiles = os.environ.get("TILES", "auto,1,2,4").split(",")
    if big:
        shapes = [(r, s, n) for r, s in ((2048, 1024), (1024, 2048), (2048, 2048), (4096, 1024)) for n in (128, 512)]
    else:
        shapes = [(s, s, n) for s in (64, 256, 512, 1024) for n in (32, 64, 128, 256, 512)]
    for rows, side, n in shapes:
        d = X.problem(min(rows, side), n, None, side + n)
        row = dict(rows=rows, side=side, n=n, lib=lib)
        for t in tiles:
            if t == "auto":
                os.environ.pop("BO_CONV_TILE", None)
            else:
                os.environ["BO_CONV_TILE"] = t
            us = [time_us(d, rows, side) for _ in range(2 if big else 1)]
            row["us_" + t] = [round(u, 1) for u, _ in us] if big else round(us[0][0], 1)
            row["sel_" + t] = us[0][1]
        os.environ.pop("BO_CONV_TILE", None)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()

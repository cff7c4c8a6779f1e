"""Time the grid-convolution path against the chunk-major kernel on square grids: graph-replayed
predict_acquire calls (2 objectives, q = 3, the selection alone), mode "auto-conv" against
"auto-noconv", microseconds per call.  The library is the one BO_AMD_LIB names.

    python scripts/gridconv_crossover.py table OUT.json      # sides 64 / 256 / 1024 x N = 32 .. 512
    python scripts/gridconv_crossover.py clustered [side=1024] [n=512] [block=128]
                                                              # points drawn from a block x block corner
    python scripts/gridconv_crossover.py point SIDE N         # one point of the table: both modes' selections
Both print JSON; `table` also writes OUT.json: per point side, n, conv_us, old_us, speedup, gate_auto,
same_selection (did the two modes pick the same top-3) and lib."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bayesopt_smart_amd as bo  # noqa: E402
from oracle import oracle_np as O  # noqa: E402
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import gridconv_model as G  # noqa: E402

REPS = 40


def problem(side, n, block, seed):
    rng = np.random.default_rng(seed)
    b = side if block is None else block
    lin = rng.choice(b * b, size=n, replace=False)
    off = 0 if block is None else (side - b) // 3
    x = np.stack([off + lin // b, off + lin % b], axis=1).astype(np.float64)
    y = rng.normal(size=(n, 2)) * 30 + 5
    pm, pv = y.mean(0), y.var(0)
    ls, betas = rng.uniform(1.5, 2.5, size=2), rng.uniform(0.5, 2.5, size=2)
    km = np.zeros((2, n, n))
    O.update_k(km, x, 0, n, pv, ls)
    return dict(x=x, y=y, pm=pm, pv=pv, ls=ls, betas=betas, Kinv=O.invert_k(n, km))


def time_us(d, side, mode):
    cands = bo.predict.CandidateSet.grid([(0, side), (0, side)])
    prepared = bo.predict.predict_acquire(d["x"], d["y"], d["Kinv"], cands, d["pm"], d["pv"], d["ls"], d["betas"],
                                          outputs=(), topq=3, mode=mode, prepare=True)
    replay = prepared.graphed()
    for _ in range(5):
        replay()
    torch.cuda.synchronize()
    best = None
    for _ in range(3):                       # the best of three rounds of REPS back-to-back replays
        t0 = time.perf_counter()
        for _ in range(REPS):
            replay()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / REPS * 1e6
        best = dt if best is None else min(best, dt)
    sel = prepared.res["top_idx"].cpu().numpy().tolist()
    return best, sel


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "table"
    lib = os.path.basename(os.environ.get("BO_AMD_LIB", "libbo_amd.so"))
    if what == "clustered":
        side = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
        n = int(sys.argv[3]) if len(sys.argv) > 3 else 512
        block = int(sys.argv[4]) if len(sys.argv) > 4 else 128
        d = problem(side, n, block, 0)
        us, sel = time_us(d, side, "auto-conv")
        print(json.dumps(dict(case="clustered", side=side, n=n, block=block, lib=lib, conv_us=round(us, 1),
                              selected=sel)), flush=True)
        return
    if what == "point":
        side, n = int(sys.argv[2]), int(sys.argv[3])
        d = problem(side, n, None, side + n)
        out = dict(case="point", side=side, n=n, lib=lib)
        cands = bo.predict.CandidateSet.grid([(0, side), (0, side)])
        for mode in ("auto-conv", "auto-noconv"):
            r = bo.predict.predict_acquire(d["x"], d["y"], d["Kinv"], cands, d["pm"], d["pv"], d["ls"], d["betas"],
                                           outputs=("acq",), topq=6, mode=mode)
            torch.cuda.synchronize()
            out[mode] = dict(top_idx=r["top_idx"].cpu().numpy().tolist(), top_val=r["top_val"].cpu().numpy().tolist())
        print(json.dumps(out), flush=True)
        return
    rows = []
    for side in (64, 256, 1024):
        for n in (32, 64, 128, 256, 512):
            d = problem(side, n, None, side + n)
            conv, s1 = time_us(d, side, "auto-conv")
            old, s2 = time_us(d, side, "auto-noconv")
            rows.append(dict(side=side, n=n, conv_us=round(conv, 1), old_us=round(old, 1),
                             speedup=round(old / conv, 2), gate_auto=bool(G.conv_planned((side, side), n, 2)),
                             same_selection=s1 == s2, lib=lib))
            print(json.dumps(rows[-1]), flush=True)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

"""Benchmark of the north-star hot path: GP predict + acquisition (Sigma-UCB "HVI") + top-q.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A plain run does what the headline figure needs and nothing else: set-up, W warm-up steps, K
timed steps, the result line (`value`, `ms_per_step`, `selected`, the config).  --full adds, after
the timed region, everything else described below: the fused kernel's own timing and `roofline`,
`select_standalone`, `cpu_baseline` and the parity fields against it.  --dump-outputs DIR writes
what the last timed step computed (DIR/<name>.npy, float64; DUMP_LIMIT_BYTES) so that two builds
can be compared output for output: the inputs are seeded and identical from run to run.

Workload (BASELINE.json configs[2], "C3"): 2-D / 2-objective toy_function
(examples/benchmark_functions.py:33-50), N_train = 512, 1,048,576 candidates per GPU on the
reference's integer 'ij' grid (bayesian_optimization.py:338-340), length scales 20, betas 2,
q = 3 (select_next_batch with the evaluated points excluded).  Strong scaling (the default): the
fixed 1,048,576-candidate grid of BASELINE's config is split into P contiguous index ranges
(distributed.shard_range), the training set independent of P; the per-rank top-q lists meet in
one RCCL all_gather.  --scaling weak: rank r scores rows [1024 r, 1024 (r + 1)) of a
(1024 P) x 1024 grid instead.

One step = one bo_predict_acquire call per rank (K^-1 packing, alpha = K^-1 (y - pm), the
fused predict/acquisition kernel writing mu, var and acq for every candidate, the top-q
merge) + the global top-q exchange + the indices on the host.  Inputs (X, y, K^-1) are
resident in HBM before the timed region.

Prints ONE JSON line (rank 0).  The --full fields: `roofline` is the fused kernel's matrix-core
throughput over its HIP-event-timed launches: `achieved` counts the MFMA flops the kernel
executes per candidate (the upper form q = 2 k.(U k) issues about half of SURVEY.md §8d's reference-formulation F), so
`frac` <= 1 is a true fraction of the datasheet peak; the reference-formulation equivalent is
reported separately as `ref_flop_equiv_tflops`.  `traffic` is the PMC-counted HBM bytes per
launch and `traffic_ratio` its ratio to the algorithmic bytes.  `cpu_baseline` times the
C/OpenMP restatement of the reference algorithm (oracle/cpu_ref.c, DGEMM on numpy's OpenBLAS)
on this process's CPU share; its acquisition array also checks the GPU's selection
(`selection_matches_cpu`, tie-aware as SURVEY.md §8c) and every acquisition value.

    python bench.py --fit [--config C3|C4|C5]

times the GP fit on the device instead: update_k + invert_k, one
compute_mll evaluation, and one full Powell hyper-parameter fit (optimize_hyperparams_mll),
at the config's N_train.
"""

from __future__ import annotations

import argparse
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_F64_MATRIX_TFLOPS = 78.6        # MI355X dense FP64 matrix peak (datasheet)
PEAK_F32_MATRIX_TFLOPS = 157.3       # MI355X dense FP32 matrix peak (datasheet; --mode fp32)
PEAK_HBM_GBPS = 8000.0

# BASELINE.json configs (SURVEY.md §8 table / §8d synthetic inputs).  C3 is the headline
# (the default); C2 / C4 / C5 are selectable with --config for their own timings.
CONFIGS = {
    "C2": dict(dim=2, n_obj=2, n_train=128, side=512, ls=20.0, q=3, kind="grid",
               workload="C2: 2D/2-obj toy_function, N_train=128, N_cand=262,144 per GPU ('ij' grid), UCB + Sigma-UCB, q=3"),
    "C3": dict(dim=2, n_obj=2, n_train=512, side=1024, ls=20.0, q=3, kind="grid",
               workload="C3: 2D/2-obj toy_function, N_train=512, N_cand=1,048,576 per GPU ('ij' integer grid), HVI (Sigma-UCB), q=3"),
    "C4": dict(dim=6, n_obj=3, n_train=1024, m=1 << 21, ls=40.0, q=3, kind="sobol",
               workload="C4: 6D/3-obj toy_function_3d, N_train=1024, N_cand=2,097,152 unscrambled Sobol in [0,300)^6 sharded over the GPUs, HVI (Sigma-UCB), q=3"),
    "C5": dict(dim=6, n_obj=3, n_train=2048, m=1 << 22, ls=40.0, q=16, kind="sobol",
               workload="C5: 6D/3-obj toy_function_3d, N_train=2048, N_cand=4,194,304 unscrambled Sobol in [0,300)^6 sharded over the GPUs, HVI (Sigma-UCB), q=16"),
}
BETA = 2.0
# C3 constants (cpu_baseline's sample is the C3 grid)
N_TRAIN, SIDE, N_OBJ, DIM, TOPQ = 512, 1024, 2, 2, 3


def flops_per_candidate(n=N_TRAIN, n_obj=N_OBJ, d=DIM):
    """F = nobj (2N^2 + 6N) + (3d - 1) N (reference formulation)."""
    return n_obj * (2 * n * n + 6 * n) + (3 * d - 1) * n


def executed_mfma_flops_per_candidate(mode, n=N_TRAIN, n_obj=N_OBJ):
    """Matrix-core flops the chunk-major kernel issues per candidate (16x16x4 f64 MFMA = 2048
    flops, 16 candidates per wave, nch = padded N / 32 chunks of 32 rows): dense issues
    16 nch^2 MFMAs per 16 candidates and objective, upper the blocks ep <= c only,
    8 nch (nch + 1) (q = 2 k.(U k), U = upper triangle of sym(K^-1))."""
    if mode == "fp32":   # 16x16x4 f32 MFMAs, 64-row chunks and E-quads: 64 MFMAs per (chunk, E-quad)
        nch = -(-n // 64)
        return n_obj * 32 * nch * (nch + 1) * 2048 // 16
    nch = -(-n // 32)
    mfmas = 16 * nch * nch if mode == "dense" else 8 * nch * (nch + 1)
    return n_obj * mfmas * 2048 // 16


def toy_function(x):
    """examples/benchmark_functions.py:33-50."""
    return np.stack([-((x[:, 0] - 150) ** 2) + 100, -((x[:, 1] - 150) ** 2) + 20], axis=1)


def toy_function_3d(x):
    """examples/benchmark_functions.py:58-73 (3 objectives from x[0..2])."""
    return np.stack([-((x[:, 0] - 150) ** 2) + 100, -((x[:, 1] - 150) ** 2) + 20,
                     -((x[:, 2] - 5) ** 2) + 120], axis=1)


def _kinv(x, pv, ls):
    """K + 1e-6 I and its inverse (update_k / invert_k, numba_kernels.py:329-403): setup only."""
    diff = x[:, None, :] - x[None, :, :]
    sq = np.einsum("ijd,ijd->ij", diff, diff)
    n = x.shape[0]
    return np.stack([np.linalg.inv(pv[o] * np.exp(-0.5 * sq / ls[o] ** 2) + 1e-6 * np.eye(n))
                     for o in range(len(pv))])


def make_config_problem(cfg, world):
    """Seeded inputs of SURVEY.md §8d.  Returns (x, y, pm, pv, ls, betas, kinv, cand) where cand
    is ('grid', rows, side) or ('sobol', CandidateSet of kind sobol)."""
    rng = np.random.default_rng(0)
    if cfg["kind"] == "grid":
        side = cfg["side"]
        rows = side * world
        lin = rng.choice(rows * side, size=cfg["n_train"], replace=False)
        x = np.stack([lin // side, lin % side], axis=1).astype(np.float64)
        y = toy_function(x)
        cand = ("grid", rows, side)
    else:
        # the unscrambled Sobol set (scipy.stats.qmc.Sobol(6, scramble=False) * 300), generated by
        # the library from the index -- on the device inside the kernel, on the host here for
        # the training points (bit-identical to scipy, tests/test_sobol.py)
        from bayesopt_smart_amd.predict import CandidateSet
        cs = CandidateSet.sobol_set(cfg["dim"], cfg["m"], scale=300.0)
        x = cs.points(rng.choice(cfg["m"], size=cfg["n_train"], replace=False))
        y = toy_function_3d(x)
        cand = ("sobol", cs)
    pm, pv = y.mean(0), y.var(0)                               # compute_prior_mean / _variance
    ls = np.full(cfg["n_obj"], cfg["ls"])
    betas = np.full(cfg["n_obj"], BETA)
    return x, y, pm, pv, ls, betas, _kinv(x, pv, ls), cand


def make_problem(world):
    """C3 problem (scripts/ablate.py, tests): (x, y, pm, pv, ls, betas, kinv, grid rows)."""
    x, y, pm, pv, ls, betas, kinv, cand = make_config_problem(CONFIGS["C3"], world)
    return x, y, pm, pv, ls, betas, kinv, cand[1]


def _cpu_model():
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def host_cpu_share():
    """(threads to use, description) -- this process's CPU share on the GPU box: the pool's
    per-GPU share as the host exports it (OMP_NUM_THREADS), else the cgroup quota, else the
    affinity mask."""
    aff = len(os.sched_getaffinity(0))
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as fh:
            q, per = fh.read().split()
            if q != "max":
                quota = max(1, int(float(q) / float(per)))
    except (OSError, ValueError):
        pass
    env = os.environ.get("OMP_NUM_THREADS")
    threads = int(env) if env and env.isdigit() and int(env) > 0 else (min(aff, quota) if quota else aff)
    threads = min(threads, aff)
    phys = None
    try:
        cores = set()
        with open("/proc/cpuinfo") as fh:
            pid = cid = None
            for line in fh:
                if line.startswith("physical id"):
                    pid = line.split(":")[1].strip()
                elif line.startswith("core id"):
                    cid = line.split(":")[1].strip()
                    cores.add((pid, cid))
        phys = len(cores) or None
    except OSError:
        pass
    desc = (f"{threads} threads = this process's CPU share (OMP_NUM_THREADS={env}, cgroup quota "
            f"{quota}, affinity {aff} logical CPUs; machine: {os.cpu_count()} logical / {phys} physical "
            f"cores, {_cpu_model()})")
    return threads, desc


def selection_check(sel_idx, cpu_acq, excluded, q):
    """The GPU's global top-q against the CPU reference's acquisition array, with SURVEY.md
    §8c's tie rule: index equality where the reference's gaps exceed 10x the tolerance, else
    the reference acq at the chosen index must equal the reference's own rank value."""
    a = np.where(excluded, -np.inf, np.asarray(cpu_acq, dtype=np.float64))
    sel = np.asarray(sel_idx, dtype=np.int64)
    sel = sel[sel >= 0]
    n_avail = int((~excluded).sum())
    if sel.size != min(q, n_avail) or excluded[sel].any():
        return False
    order = np.argsort(-a, kind="stable")[: q + 1]
    top = a[order]
    tol = 1e-5 * np.maximum(1.0, np.abs(top))
    for t in range(sel.size):
        gap = t + 1 < top.size and top[t] - top[t + 1] > 10 * tol[t] and (t == 0 or top[t - 1] - top[t] > 10 * tol[t])
        if gap and sel[t] != order[t]:
            return False
        if not gap and abs(a[sel[t]] - top[t]) > 2 * tol[t]:
            return False
    return True


DUMP_LIMIT_BYTES = 64 * 1000 * 1000     # --dump-outputs: all files of one rank together


def dump_sample_index(n_cand, values_per_cand, limit=DUMP_LIMIT_BYTES, seed=0):
    """--dump-outputs: the candidate columns written.  None = all of them (the arrays fit into
    `limit` bytes as float64); else a fixed ascending sample of the candidate index, drawn with
    `seed`, so large that values_per_cand float64 values per sampled candidate plus the sample's
    own index array fit -- the same columns for every build and run.  64 KiB of the limit are
    kept for the selection (at most BO_MAX_TOPQ = 48 points) and the .npy headers."""
    limit -= 1 << 16
    if 8 * values_per_cand * n_cand <= limit:
        return None
    k = limit // (8 * (values_per_cand + 1))
    return np.sort(np.random.default_rng(seed).choice(n_cand, size=int(k), replace=False))


def dump_outputs(path, out, sel, suffix=""):
    """--dump-outputs: the arrays a caller of the timed step receives, as left by the last timed
    step -- every per-candidate output (`out`: name -> device tensor [..., n_cand]) and the step's
    returned selection -- as float64 .npy files (`sample_index.npy` when the candidates are
    sampled; the selection indices are exact in float64).  All files of one call together stay
    within DUMP_LIMIT_BYTES."""
    os.makedirs(path, exist_ok=True)
    n_cand = next(iter(out.values())).shape[-1]
    idx = dump_sample_index(n_cand, sum(t.numel() // n_cand for t in out.values()))
    save = lambda name, a: np.save(os.path.join(path, f"{name}{suffix}.npy"),  # noqa: E731
                                   np.ascontiguousarray(a, dtype=np.float64))
    if idx is not None:
        save("sample_index", idx)
    for name, t in out.items():
        a = t.cpu().numpy()
        save(name, a if idx is None else a[..., idx])
    save("selected_values", sel[0])
    save("selected_indices", sel[1])


def cpu_baseline(x, y, pm, pv, ls, betas, kinv, points, label, q, max_cand=SIDE * SIDE, chunk=32768,
                 passes=5, pass_s=3.0, full_limit=1 << 21):
    """Reference algorithm on the host cores: oracle/cpu_ref.c, the C/OpenMP restatement of
    update_k_star -> update_mean -> update_variance (materialised K* per candidate block,
    DGEMM K^-1 K*, the serial quadratic form) -> standardise -> UCB -> Sigma-UCB, then
    select_next_batch's full descending sort + exclusion walk.
    points(lo, hi) -> f64 [hi - lo, d] candidates of the workload.

    Timing: one untimed warm-up chunk, then `passes` timed passes over a
    sample of the first S candidates (S sized for ~pass_s seconds per pass, at most the shard);
    value = S / median pass time.  For the parity fields the rest of the shard is then scored
    untimed when it has at most `full_limit` candidates (all of C2/C3/C4; --cpu-full for C5)."""
    from oracle import cpu_ref
    threads, share = host_cpu_share()
    cpu_ref.load()
    run = lambda lo, hi: cpu_ref.predict_acquire(x, y, points(lo, hi), kinv, pm, pv, ls, betas,  # noqa: E731
                                                 threads=threads, outputs=True)["acq"]
    w = min(chunk, max_cand)
    t0 = time.perf_counter()
    run(0, w)                                            # warm-up (thread pool, BLAS)
    rate = w / max(time.perf_counter() - t0, 1e-9)
    sample = int(min(max_cand, max(w, (rate * pass_s) // chunk * chunk)))
    times, acq = [], None
    for _ in range(passes):
        t0 = time.perf_counter()
        acq = np.concatenate([run(lo, min(lo + chunk, sample)) for lo in range(0, sample, chunk)])
        times.append(time.perf_counter() - t0)
    t_med = float(np.median(times))
    done = sample
    if sample < max_cand and max_cand <= full_limit:     # untimed: the rest, for the parity fields
        parts, t_log = [acq], time.perf_counter()
        for lo in range(sample, max_cand, chunk):
            parts.append(run(lo, min(lo + chunk, max_cand)))
            if time.perf_counter() - t_log > 30.0:      # progress of a long untimed scoring (C5 --cpu-full)
                print(f"[bench] cpu reference: {lo + chunk} of {max_cand} candidates scored", file=sys.stderr, flush=True)
                t_log = time.perf_counter()
        acq = np.concatenate(parts)
        done = max_cand
    cpu_sel = cpu_ref.select(acq, points(0, done), x, q)
    res = {"value": sample / t_med, "unit": "candidate-points/sec", "cores": threads, "kind": "port",
           "sample": f"{'all' if sample == max_cand else 'first'} {sample} candidates of the {label} "
                     f"(N_train={x.shape[0]}, {len(pm)} objectives, mu/var/acq written), median of {passes} "
                     f"timed passes ({', '.join(f'{t:.2f}' for t in times)} s) after a {w}-candidate warm-up; "
                     f"oracle/cpu_ref.c (C/OpenMP, DGEMM: {cpu_ref.dgemm_name()}), {share}; "
                     f"{done} candidates scored for the parity fields"}
    return res, acq, cpu_sel


def _lib_sha256():
    """sha256 of the loaded libbo_amd.so (the binary a PMC summary must come from)."""
    import hashlib
    from bayesopt_smart_amd import _lib
    with open(_lib.LIB_PATH, "rb") as fh:
        return hashlib.sha256(fh.read()).hexdigest()


def device_code_sha256(path):
    """sha256 of a library's device code: the bytes of its .hip_fatbin ELF section (every gfx950
    code object the kernels run from).  A relink of the same objects -- or a rebuild of the same
    sources at the same path -- leaves it unchanged where the file's own sha256 may differ in host
    bytes; None if the section is missing."""
    import hashlib
    import struct
    with open(path, "rb") as fh:
        data = fh.read()
    if data[:4] != b"\x7fELF" or data[4] != 2:                       # ELF64 only
        return None
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", data, 0x3A)
    sec = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    stro = sec[shstrndx][4]
    for name, _typ, _fl, _addr, off, size, *_ in sec:
        end = data.index(b"\0", stro + name)
        if data[stro + name:end] == b".hip_fatbin":
            return hashlib.sha256(data[off:off + size]).hexdigest()
    return None


def pmc_traffic(workload="C3"):
    """HBM bytes per fused-kernel launch from a committed rocprofv3 PMC summary of this workload
    (profiles/*pmc*.json, scripts/pmc_summary.py) taken with THIS library's kernels: its file
    sha256 (lib_sha256), or the sha256 of its device code (fatbin_sha256, device_code_sha256) --
    the counters count the kernels, and a relink that changes only host bytes keeps them.  None
    when no summary of these kernels exists (a summary of another build is never used)."""
    from bayesopt_smart_amd import _lib
    sha = _lib_sha256()
    fsha = device_code_sha256(_lib.LIB_PATH)
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*pmc*.json")))
    for f in reversed(files):
        try:
            with open(f) as fh:
                d = json.load(fh)
            same = d.get("lib_sha256") == sha or (fsha is not None and d.get("fatbin_sha256") == fsha)
            if d.get("workload") == workload and d.get("hbm_bytes_per_launch") and same:
                return float(d["hbm_bytes_per_launch"]), os.path.basename(f)
        except Exception:
            pass
    return None, None


def run_fit(cfg, label, dev):
    """--fit: the GP fit on the device at the config's N_train.
    update_k + invert_k (numba_kernels.py:329-403), one compute_mll (:152-235), one Powell fit
    (optimize_hyperparams_mll, :238-321: every MLL evaluation one device call).  Each timing is
    the median of repeated calls, synchronised; parity against numpy/LAPACK is reported beside."""
    import torch
    import bayesopt_smart_amd as bo
    from oracle import oracle_np as O
    x, y, pm, pv, ls, betas, kinv_ref, _ = make_config_problem(cfg, 1)
    n, n_obj = x.shape[0], len(pm)
    xd = torch.tensor(x, device=dev)
    yd = torch.tensor(y, device=dev)
    km = torch.zeros((n_obj, n, n), dtype=torch.float64, device=dev)

    def timed(fn, reps):
        ts, out = [], None
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)) * 1e3, out

    def gram_inverse():
        bo.kernels.update_k(km, xd, 0, n, pv, ls)
        return bo.kernels.invert_k(n, km)

    gram_inverse()
    inv_ms, kinv = timed(gram_inverse, 5)
    kinv = kinv.cpu().numpy()
    inv_err = float(np.abs(kinv - kinv_ref).max() / np.abs(kinv_ref).max())
    mll_fn = lambda: bo.kernels.compute_mll(xd, yd, km, pm, pv, ls, n)  # noqa: E731
    mll_fn()
    mll_ms, mll = timed(mll_fn, 10)
    km_h = np.zeros((n_obj, n, n))
    mll_ref = O.compute_mll(x, y, km_h, pm, pv, ls, n)
    # the LU path (bo_lu.hip): objective 0's K made non-symmetric forces it (Cholesky skipped)
    rng = np.random.default_rng(3)
    km_lu = km.clone()
    km_lu[0] += torch.tensor(np.triu(rng.uniform(-1e-3, 1e-3, size=(n, n)) * pv[0], 1), device=dev)
    lu_fn = lambda: bo.kernels.invert_k(n, km_lu)  # noqa: E731
    c0 = bo._lib.invert_k_path_counts()
    lu_fn()
    lu_ms, kinv_lu = timed(lu_fn, 3)
    c1 = bo._lib.invert_k_path_counts()
    ref_lu = np.linalg.inv(km_lu[0].cpu().numpy() + 1e-6 * np.eye(n))
    lu_err = float(np.abs(kinv_lu[0].cpu().numpy() - ref_lu).max() / np.abs(ref_lu).max())
    ls_fit, pv_fit = ls.copy(), pv.copy()
    paths0 = bo._lib.fit_path_counts()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = bo.kernels.optimize_hyperparams_mll(xd, yd, km, pm, pv_fit, ls_fit, n)
    torch.cuda.synchronize()
    fit_ms = (time.perf_counter() - t0) * 1e3
    paths1 = bo._lib.fit_path_counts()
    # the same fit with scipy's Powell driver over the same device terms (the round-3 path)
    ls_s, pv_s = ls.copy(), pv.copy()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res_s = bo.kernels.optimize_hyperparams_mll(xd, yd, km, pm, pv_s, ls_s, n, driver="scipy")
    torch.cuda.synchronize()
    fit_scipy_ms = (time.perf_counter() - t0) * 1e3
    return {
        "metric": f"GP fit on device (Gram + inverse, MLL evaluation, Powell fit), {label}",
        "value": fit_ms, "unit": "ms per Powell hyper-parameter fit", "higher_is_better": False,
        "n_gpus": 1, "dtype": "f64", "data": "synthetic (the bench workload's training set)",
        "config": {"workload": cfg["workload"], "n_train": n, "n_objectives": n_obj, "dim": x.shape[1]},
        "update_k_invert_k_ms": inv_ms, "invert_k_rel_err_vs_lapack": inv_err,
        "invert_k_lu_path_ms": lu_ms, "invert_k_lu_path_rel_err_vs_lapack": lu_err,
        "invert_k_lu_path_note": (f"objective 0 non-symmetric -> blocked LU + getrs; objective 1 "
                                  f"Cholesky; paths taken per timed call: "
                                  f"{ {k: (c1[k] - c0[k]) / 4 for k in c1} }"),
        "compute_mll_ms": mll_ms, "mll": mll, "mll_lapack": mll_ref,
        "mll_rel_err": abs(mll - mll_ref) / max(1.0, abs(mll_ref)),
        "powell_nfev": int(res.nfev), "powell_ms_per_eval": fit_ms / max(int(res.nfev), 1),
        "powell_device_calls": int(getattr(res, "device_calls", -1)),
        "powell_driver": "native (bo_optimize_hyperparams_mll: one library call)",
        "powell_scipy_driver_ms": fit_scipy_ms,
        "powell_scipy_driver_same_result": bool(np.array_equal(res.x, res_s.x) and res.nfev == res_s.nfev),
        "factorisation_schedule": os.environ.get("BO_FIT_PATH", "persistent"),
        "fit_paths_during_powell": {k: paths1[k] - paths0[k] for k in paths1},
        "fitted_length_scales": ls_fit.tolist(),
    }


def run_fit_demo(n_max, dev):
    """--fit-demo: how often invert_k leaves the Cholesky path in a headless demo-style run
    (examples/demo_2d.py: toy_function on the 300 x 300 grid, 6 initial points, batches of 3,
    hyper-parameters Powell-fitted every iteration as the reference's loop does,
    bayesian_optimization.py:115-123) up to N = n_max training points."""
    import bayesopt_smart_amd as bo

    def toy(p):
        p = np.asarray(p, dtype=np.float64)
        return np.array([-((p[0] - 150) ** 2) + 100.0, -((p[1] - 150) ** 2) + 20.0])

    iters = (n_max - 6) // 3
    c0 = bo._lib.invert_k_path_counts()
    t0 = time.perf_counter()
    opt = bo.BayesianOptimization(toy, [(0, 300), (0, 300)], n_objectives=2, n_iterations=iters,
                                  initial_samples=6, batch_size=3, device=dev)
    opt.optimize()
    dt = time.perf_counter() - t0
    c1 = bo._lib.invert_k_path_counts()
    d = {k: c1[k] - c0[k] for k in c1}
    tot = sum(d.values())
    return {"metric": "invert_k path frequency in a demo-style run (Powell-fitted hyper-parameters)",
            "value": d["lu"] + d["gauss_jordan"], "unit": f"objective inversions off the Cholesky path (of {tot})",
            "higher_is_better": False, "n_gpus": 1, "data": "toy_function on the 300 x 300 grid",
            "config": {"initial_samples": 6, "batch_size": 3, "iterations": iters, "n_train_final": 6 + 3 * iters},
            "paths": d, "fallback_fraction": (d["lu"] + d["gauss_jordan"]) / max(tot, 1),
            "fitted_length_scales": opt.length_scales.tolist(), "run_s": dt,
            "best_found": opt.x_vector[np.argmax(opt.y_vector[: opt.n_evaluations, 0])].tolist()}


# The reference's only published timings (BayesianOptimization_Tutorial.ipynb, Numba CPU, host
# unstated): the headless demo (toy_function, 300 x 300 grid, 6 initial points, batches of 3, 15
# iterations, betas 2), per-iteration `timings` (bayesian_optimization.py:236-242) in seconds.
C1_REF = {"n6": {"hyperparams": 0.0163, "kernels": 0.0171, "acquisition": 0.0169, "source": "ipynb:244"},
          "n48": {"hyperparams": 0.0134, "kernels": 0.0306, "acquisition": 0.0498, "source": "ipynb:384"},
          "avg": {"hyperparams": 0.0123, "kernels": 0.0187, "acquisition": 0.0294, "source": "ipynb:432-434"}}
C1_M = 300 * 300


def _toy_point(p):
    p = np.asarray(p, dtype=np.float64)
    return np.array([-((p[0] - 150) ** 2) + 100.0, -((p[1] - 150) ** 2) + 20.0])


def _toy3_point(p):
    return toy_function_3d(np.asarray(p, dtype=np.float64)[None])[0]


def run_c1(dev, repeats=3):
    """--config C1: the reference's demo (BASELINE.json configs[0]; examples/demo_2d.py, the
    notebook's cell 8: toy_function on the 300 x 300 grid, initial_samples 6, batch_size 3,
    n_iterations 15, betas 2) through the drop-in BayesianOptimization, with the reference's
    per-iteration `timings` from a callback.  One untimed warm-up run (library load, workspace
    allocation, first launches), then `repeats` timed runs of the same seeded trajectory (the LHS
    design is the reference's, np.random.seed(42)); per iteration the median over the runs.
    value = candidates / (kernels + acquisition), averaged over the 15 iterations, as the
    notebook's numbers give it (ipynb:432-434); vs_baseline = that / the notebook's average."""
    import bayesopt_smart_amd as bo

    def one_run():
        np.random.seed(42)
        recs = []
        opt = bo.BayesianOptimization(_toy_point, [(0, 300), (0, 300)], n_objectives=2, initial_samples=6,
                                      n_iterations=15, batch_size=3, betas=np.array([2.0, 2.0]), device=dev,
                                      callbacks=[lambda st: recs.append(dict(st["timings"], n=int(st["iteration"]),
                                                                             x_next=np.array(st["x_next"]).tolist()))])
        t0 = time.perf_counter()
        opt.optimize()
        return recs, opt, time.perf_counter() - t0

    one_run()
    runs = [one_run() for _ in range(repeats)]
    keys = ("hyperparams", "kernels", "acquisition", "eval", "total")
    per_it = []
    for i, r0 in enumerate(runs[0][0]):
        per_it.append({"n_train": r0["n"], **{k: float(np.median([r[0][i][k] for r in runs])) for k in keys}})
    for r in runs[1:]:
        assert [x["x_next"] for x in r[0]] == [x["x_next"] for x in runs[0][0]], "trajectory changed between runs"
    avg = {k: float(np.mean([p[k] for p in per_it])) for k in keys}
    rate = lambda d: C1_M / (d["kernels"] + d["acquisition"])  # noqa: E731
    ref_avg_rate = rate(C1_REF["avg"])
    first, last = per_it[0], per_it[-1]
    opt = runs[0][1]
    return {
        "metric": "candidate-points/sec (GP predict + acquisition: the reference's kernels + acquisition "
                  "stages), BASELINE config C1 (the reference's published demo)",
        "value": rate(avg), "unit": "candidate-points/sec", "higher_is_better": True, "n_gpus": 1,
        "vs_baseline": rate(avg) / ref_avg_rate,
        "baseline": {"value": ref_avg_rate, "source": "BayesianOptimization_Tutorial.ipynb:432-434 (Numba CPU, "
                     "host unstated): 90,000 / (0.0187 + 0.0294) s, the 15-iteration average"},
        "dtype": "f64", "data": "toy_function (examples/benchmark_functions.py:33-50), the reference's LHS design",
        "config": {"workload": "C1: demo_2d, 2-D/2-obj, 300 x 300 grid (M = 90,000), initial 6, batch 3, "
                               "15 iterations (N = 6 -> 48), betas 2", "parallelism": "x1"},
        "timings_s": {"n6": first, "n48": last, "avg": avg},
        "reference_timings_s": C1_REF,
        "vs_reference": {
            "n6_kernels_plus_acquisition": (C1_REF["n6"]["kernels"] + C1_REF["n6"]["acquisition"]) /
                                           (first["kernels"] + first["acquisition"]),
            "n48_kernels_plus_acquisition": (C1_REF["n48"]["kernels"] + C1_REF["n48"]["acquisition"]) /
                                            (last["kernels"] + last["acquisition"]),
            "avg_kernels_plus_acquisition": (C1_REF["avg"]["kernels"] + C1_REF["avg"]["acquisition"]) /
                                            (avg["kernels"] + avg["acquisition"]),
            "avg_hyperparams": C1_REF["avg"]["hyperparams"] / avg["hyperparams"],
            "note": "speed-up factors (reference time / this time); the stage split differs: the reference's "
                    "'kernels' holds update_k + invert_k + update_k_star and 'acquisition' the mean, variance, "
                    "UCB, HVI and select; here 'kernels' is update_k + invert_k and 'acquisition' the fused "
                    "predict + select, so their SUM is the comparable figure"},
        "cand_per_s": {"n6": rate(first), "n48": rate(last), "avg": rate(avg)},
        "per_iteration": per_it,
        "run_s": [r[2] for r in runs],
        "best_found": opt.x_vector[np.argmax(opt.y_vector[: opt.n_evaluations, 0])].tolist(),
        "fitted_length_scales": opt.length_scales.tolist(),
    }


def run_iteration(cfg_name, cfg, dev, args, world, rank):
    """--iteration: the drop-in loop (optimize(), bayesian_optimization.py:108-247) at the config's
    N_train on the config's candidates: hyper-parameter fit (native Powell over the device MLL;
    COBYLA in the float32 branch), update_k + invert_k, the fused predict + acquisition + select,
    the objective on the new batch.  `warmup` + `steps` iterations from the config's seeded
    design; per iteration the reference's `timings` keys from a callback; medians over the timed
    ones (N grows by q per iteration).  C5 runs in its stated float32 branch (--mode auto for f64)."""
    import bayesopt_smart_amd as bo
    from bayesopt_smart_amd.bayesian_optimization import optimize
    x, y, pm, pv, ls, betas, _, cand = make_config_problem(cfg, 1)
    n, q, d, n_obj = cfg["n_train"], cfg["q"], cfg["dim"], cfg["n_obj"]
    ft = np.float32 if args.mode == "fp32" else np.float64
    iters = args.warmup + args.steps
    total = n + q * iters
    if cand[0] == "grid":
        cands = bo.CandidateSet.grid([(0, cand[1]), (0, cand[2])])
        fn = _toy_point
    else:
        cands = cand[1]
        fn = _toy3_point
    xv = np.zeros((total, d), dtype=ft)
    yv = np.zeros((total, n_obj), dtype=ft)
    xv[:n], yv[:n] = x, y
    lsv, pvv = ls.astype(ft), pv.astype(ft)
    recs = []
    cb = [lambda st: recs.append(dict(st["timings"], n=int(st["iteration"])))]
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    optimize(xv, yv, None, None, None, None, None, None, None, None, cands, pm.astype(ft), pvv, None, n, total,
             n_obj, fn, betas.astype(ft), lsv, q, None, callbacks=cb, float_type=ft)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    timed = recs[args.warmup:]
    keys = ("hyperparams", "kernels", "acquisition", "eval", "total")
    med = {k: float(np.median([r[k] for r in timed])) for k in keys}
    return {
        "metric": f"drop-in loop iteration (fit + update_k/invert_k + predict + acquisition + select), {cfg_name}",
        "value": med["total"] * 1e3, "unit": "ms per iteration (median)", "higher_is_better": False,
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "dtype": "f32" if ft == np.float32 else "f64",
        "data": "synthetic (the bench workload's seeded design and objective)",
        "config": {"workload": cfg["workload"], "n_train_first": n, "n_train_last": n + q * (iters - 1),
                   "batch": q, "float_type": "float32" if ft == np.float32 else "float64",
                   "parallelism": f"candidate-shard x{world}"},
        "timings_ms": {k: v * 1e3 for k, v in med.items()},
        "per_iteration_ms": [{"n_train": r["n"], **{k: r[k] * 1e3 for k in keys}} for r in recs],
        "fitted_length_scales": np.asarray(lsv, dtype=np.float64).tolist(),
        "wall_s": wall,
        "note": "timings keys as bayesian_optimization.py:236-242: hyperparams = the Powell (COBYLA) fit; "
                "kernels = update_k + invert_k; acquisition = the fused predict + acquisition + top-q (+ the "
                "exchange with several ranks); eval = the objective on the batch",
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", choices=sorted(CONFIGS) + ["C1"], default="C3",
                    help="BASELINE.json config (C3 = the headline metric; C1 = the reference's published demo, "
                         "through BayesianOptimization with the reference's timings)")
    ap.add_argument("--iteration", action="store_true",
                    help="time whole drop-in loop iterations (fit + kernels + acquisition + eval) at the config")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure and check what the headline figure does not "
                         "need: the fused kernel's own timing (roofline), select_standalone, cpu_baseline "
                         "and the parity fields against it")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed (every per-candidate output array and "
                         "the selection) as DIR/<name>.npy in float64, at most 64 MB in all (a fixed "
                         "seeded sample of the candidates above that)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the cpu_baseline leg")
    ap.add_argument("--cpu-full", action="store_true",
                    help="--full: score the whole shard on the CPU for the parity fields even above 2^21 "
                         "candidates (C5: minutes of host time, outside the timed region)")
    ap.add_argument("--no-graph", action="store_true", help="launch the step's kernels directly "
                    "instead of replaying them as one HIP graph")
    ap.add_argument("--fit", action="store_true", help="time the device GP fit instead (SURVEY §8f)")
    ap.add_argument("--fit-demo", type=int, default=0, metavar="N_MAX",
                    help="count invert_k's Cholesky / LU paths in a demo-style run up to N_MAX points")
    ap.add_argument("--mode", choices=("auto", "dense", "fp32"), default=None,
                    help="variance formulation (auto = 2 k.(U k) with U = triu(sym(K^-1)), diagonal halved); "
                         "fp32 = the same form on the f32 matrix cores; default: fp32 for C5 (BASELINE: "
                         "'8xMI355X fp32 with fp64 reference check'), auto otherwise")
    ap.add_argument("--scaling", choices=("strong", "weak"), default=None,
                    help="strong (default): the config's fixed candidate set split over the GPUs; "
                         "weak (grid configs): every GPU scores a full-size grid block")
    ap.add_argument("--acq", choices=("sum_ucb", "hvi"), default="sum_ucb",
                    help="sum_ucb = the reference's 'hypervolume improvement' (sum of UCBs, fused top-q); "
                         "hvi = exact hypervolume improvement over the evaluated Pareto front (extension)")
    ap.add_argument("--hvi-unmasked", action="store_true",
                    help="--acq hvi: exclude the evaluated points per call (hash set) instead of the "
                         "persistent exclusion mask")
    args = ap.parse_args()
    if args.mode is None:
        args.mode = "fp32" if args.config == "C5" else "auto"
    cfg = CONFIGS.get(args.config)
    if args.dump_outputs and (args.config == "C1" or args.iteration or args.fit or args.fit_demo):
        raise SystemExit("--dump-outputs writes the predict + acquisition step's outputs "
                         "(not --config C1, --iteration, --fit, --fit-demo)")

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    # BO_BENCH_BACKEND=gloo: a functional rehearsal of the multi-rank step with several ranks on
    # one device (not a measurement); the product launch is one rank per GPU over RCCL
    backend = os.environ.get("BO_BENCH_BACKEND", "nccl")
    # BO_FORCE_COLLECTIVES=1 with WORLD_SIZE=1 (torch.distributed.run --nproc-per-node 1): the
    # process group and every exchange of the step run on one rank (tests/test_gpu_rccl_one_rank.py)
    use_dist = world > 1 or os.environ.get("BO_FORCE_COLLECTIVES") == "1"
    if backend != "nccl":
        local %= max(1, torch.cuda.device_count())
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if args.config == "C1":
        if world > 1:
            raise SystemExit("--config C1 is the reference's single-process demo")
        print(json.dumps(run_c1(dev)), flush=True)
        return
    if args.iteration:
        if use_dist:
            dist.init_process_group("nccl" if backend == "nccl" else backend,
                                    **({"device_id": dev} if backend == "nccl" else {}))
        res = run_iteration(args.config, cfg, dev, args, world, rank)
        if rank == 0:
            print(json.dumps(res), flush=True)
        if use_dist:
            dist.destroy_process_group()
        return
    if args.fit or args.fit_demo:
        if world > 1:
            raise SystemExit("--fit / --fit-demo are single-GPU measurements")
        print(json.dumps(run_fit_demo(args.fit_demo, dev) if args.fit_demo else run_fit(cfg, args.config, dev)),
              flush=True)
        return
    if use_dist:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    import bayesopt_smart_amd as bo
    from bayesopt_smart_amd.distributed import shard_range
    lib = bo._lib.load()

    scaling = args.scaling or "strong"
    if scaling == "weak" and cfg["kind"] != "grid":
        raise SystemExit("--scaling weak applies to the grid configs (C2/C3)")
    x, y, pm, pv, ls, betas, kinv, cand = make_config_problem(cfg, world if scaling == "weak" else 1)
    n_obj, q = cfg["n_obj"], cfg["q"]
    if cand[0] == "grid" and scaling == "strong":
        # strong scaling: the fixed side x side grid split into P balanced contiguous index ranges
        side = cand[2]
        cands = bo.CandidateSet.grid([(0, cand[1]), (0, side)])
        total = cands.n
        offset, per_rank = shard_range(total, rank, world)
    elif cand[0] == "grid":
        # weak scaling: rank r owns grid rows [side r, side (r + 1)) of a (side P) x side grid
        side = cand[2]
        cands = bo.CandidateSet.grid([(0, cand[1]), (0, side)])
        per_rank = side * side
        offset = rank * per_rank
        total = world * per_rank
    else:
        # strong scaling: the fixed Sobol set split into P balanced contiguous index ranges; each
        # rank's kernel generates its own range from the index (no candidate array anywhere)
        cands = cand[1]
        m = cands.n
        offset, per_rank = shard_range(m, rank, world)
        total = m
    xd = torch.tensor(x, device=dev)
    yd = torch.tensor(y, device=dev)
    kd = torch.tensor(kinv, device=dev)
    outputs = ("mu", "var", "ucb", "acq") if args.config == "C2" or args.acq == "hvi" else ("mu", "var", "acq")
    out = {k: torch.empty((per_rank,) if k == "acq" else (n_obj, per_rank), dtype=torch.float64,
                          device=dev) for k in outputs}
    # the top-q exchange: each rank's list as ONE block of 16-B records (values, int64 indices),
    # one all_gather of P * q * 16 bytes
    # (one shard: the record block lives in pinned host memory and the merge kernel writes the
    # selection straight into it -- no device-to-host copy launch per step)
    rec = torch.empty(2 * q, dtype=torch.float64, device=dev) if use_dist or args.acq == "hvi" \
        else torch.empty(2 * q, dtype=torch.float64).pin_memory()
    rec_np = rec.numpy() if rec.device.type == "cpu" else None
    gath = torch.empty(world * 2 * q, dtype=torch.float64, device=dev)
    # the gathered records land in a preallocated pinned buffer (one async copy + a stream
    # synchronisation per step instead of a pageable allocation and copy)
    gath_h = torch.empty(world * 2 * q, dtype=torch.float64).pin_memory()
    gath_np = gath_h.numpy().reshape(world, 2 * q)

    hvi_ev = []
    if args.acq == "hvi":
        # exact HVI: the UCB vectors of this shard against the Pareto front of the evaluated
        # objectives, reference point below every observation; then the standalone top-q
        import ctypes
        from bayesopt_smart_amd.acquisition import hypervolume_boxes
        ref_pt = y.min(axis=0) - 1.0
        front_y = y[bo.is_pareto_efficient(y)]
        exd = torch.tensor(x, device=dev)
        sel_ws = torch.empty(lib.bo_select_topq_workspace_size(per_rank, q), dtype=torch.uint8, device=dev)
        glo = (ctypes.c_int64 * 8)(*((list(cands.lo) if cands.lo else []) + [0] * (8 - len(cands.lo or []))))
        gsh = (ctypes.c_int64 * 8)(*((list(cands.shape) if cands.shape else []) + [1] * (8 - len(cands.shape or []))))
        shift = (ctypes.c_double * n_obj)(*pm[:n_obj])
        scale = (ctypes.c_double * n_obj)(*np.sqrt(pv[:n_obj]))
        strm = bo.device.stream_handle(dev)
        n_boxes = [0]
        # the evaluated points' exclusion mask of this shard (bo_excl_mask_update), as the loop
        # keeps it: built once, then extended by each iteration's q new points (both timed here,
        # outside the step; reported in hvi_select)
        from bayesopt_smart_amd.acquisition import ExclusionMask
        hvi_mask = ExclusionMask(cands, offset, per_rank, dev)
        mask_ms = {}
        for tag, rows in (("build_ms", x[:-q]), ("extend_q_ms", x)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            hvi_mask.update(rows)
            e1.record()
            torch.cuda.synchronize()
            mask_ms[tag] = e0.elapsed_time(e1)

        def step_hvi():
            # fused predict writing the UCB arrays, the box decomposition of the non-dominated
            # region (host), then ONE pass computing the exact HVI of every candidate and its
            # top-q with exclusion (bo_hvi_select_topq_masked over the shard's exclusion mask;
            # --hvi-unmasked: bo_hvi_select_topq with the points), event-timed
            bo.predict_acquire(xd, yd, kd, cands, pm, pv, ls, betas, outputs=outputs, topq=0,
                               offset=offset, count=per_rank, out=out, device=dev, mode=args.mode)
            boxes = torch.as_tensor(hypervolume_boxes(front_y, ref_pt), device=dev)
            n_boxes[0] = boxes.shape[0]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if args.hvi_unmasked:
                bo._lib.check(lib.bo_hvi_select_topq(
                    out["acq"].data_ptr(), out["ucb"].data_ptr(), per_rank, per_rank, n_obj, shift, scale,
                    boxes.data_ptr(), boxes.shape[0], cands.kind_code,
                    (cands.tensor[offset:].data_ptr() if cands.kind in ("i64", "f64") else cands.cand_arg),
                    glo, gsh, cands.dim, offset, exd.data_ptr(), exd.shape[0], q, rec.data_ptr(),
                    rec.data_ptr() + 8 * q, sel_ws.data_ptr(), sel_ws.numel(), strm), "hvi_select")
            else:
                bo._lib.check(lib.bo_hvi_select_topq_masked(
                    out["acq"].data_ptr(), out["ucb"].data_ptr(), per_rank, per_rank, n_obj, shift, scale,
                    boxes.data_ptr(), boxes.shape[0], offset, hvi_mask.ptr, q, rec.data_ptr(),
                    rec.data_ptr() + 8 * q, sel_ws.data_ptr(), sel_ws.numel(), strm), "hvi_select_masked")
            e1.record()
            hvi_ev.append((e0, e1))

    # the validated call, launched once per step (a plan object: every launch re-runs the
    # preparation -- W packing, alpha, rows --, the fused kernel and its top-q merge)
    predict = bo.predict_acquire(xd, yd, kd, cands, pm, pv, ls, betas, outputs=outputs, topq=q,
                                 offset=offset, count=per_rank, out=out, device=dev, mode=args.mode,
                                 top_rec=rec, prepare=True)

    # the prepared call replayed as a HIP graph (one launch per step from the host); the
    # library's kernel timer runs over separate non-graph calls after the timed region
    run, step_launch = predict, "direct"
    if args.acq != "hvi" and not args.no_graph:
        try:
            run, step_launch = predict.graphed(), "hip_graph"
        except Exception as exc:  # capture unsupported here: launch directly (stated in the line)
            print(f"[bench] HIP graph capture failed ({exc}); launching directly", file=sys.stderr)

    def step():
        if args.acq == "hvi":
            step_hvi()
        else:
            run()
        if use_dist:
            if backend == "nccl":
                dist.all_gather_into_tensor(gath, rec)
                gath_h.copy_(gath, non_blocking=True)
                torch.cuda.current_stream(dev).synchronize()
            else:
                dist.all_gather_into_tensor(gath_h, rec.cpu())
            return bo.merge_topq(gath_np[:, :q], gath_np[:, q:].view(np.int64), q)
        # one shard: the device list is already merged and in selection order
        if rec_np is not None:
            torch.cuda.current_stream(dev).synchronize()
            v, i = rec_np[:q].copy(), rec_np[q:].view(np.int64).copy()
        else:
            g = rec.cpu()
            v, i = g[:q].numpy(), g[q:].view(torch.int64).numpy()
        return v[i >= 0], i[i >= 0]

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    graphed = run is not predict
    if not graphed:
        lib.bo_profile_start(args.steps)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        sel = step()
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    # this rank's own fused top-q (before the exchange): what its standalone selection must match
    local_sel = rec.cpu()[q:].view(torch.int64).numpy() if use_dist else np.asarray(sel[1])
    local_sel = local_sel[local_sel >= 0]
    dt = time.perf_counter() - t0
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, out, sel, f"_rank{rank}" if world > 1 else "")
    import ctypes
    kms, nl = ctypes.c_double(), ctypes.c_int()
    if graphed and args.full:
        # the fused kernel's launch duration: HIP events on its stream over as many direct calls
        lib.bo_profile_start(args.steps)
        for _ in range(args.steps):
            predict()
        torch.cuda.synchronize()
    # the kernel's own time: from the timed steps themselves when they were direct launches, from
    # --full's extra direct calls when they were graph replays (a plain graphed run has none)
    kernel_timed = args.full or not graphed
    if kernel_timed:
        lib.bo_profile_stop(ctypes.byref(kms), ctypes.byref(nl))
    t_step = dt / args.steps
    hv_front = None
    if args.acq == "hvi":
        # the hypervolume accumulator: the front's box decomposition split over the ranks, one
        # all_reduce (RCCL) -- outside the timed region, reported beside the selection
        from bayesopt_smart_amd.distributed import front_hypervolume
        hv_front = front_hypervolume(front_y, ref_pt, device=dev)
    if use_dist:
        tt = torch.tensor([t_step, kms.value / max(nl.value, 1)], dtype=torch.float64,
                          device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        t_step, k_ms = tt.tolist()
    else:
        k_ms = kms.value / max(nl.value, 1)

    if rank == 0:
        n, d = cfg["n_train"], cfg["dim"]
        metric = ("candidate-points/sec (GP predict + HVI) at N_train=512, N_cand=1M" if args.config == "C3"
                  else f"candidate-points/sec (GP predict + HVI), BASELINE config {args.config}")
        if args.acq == "hvi":
            metric += " [acquisition: exact hypervolume improvement, not the reference's sum of UCBs]"
        res = {
            "metric": metric,
            "value": total / t_step,
            "unit": "candidate-points/sec",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": t_step * 1e3,
            "higher_is_better": True,
            "scaling": scaling,
            "vs_baseline": None,
            "dtype": "f32" if args.mode == "fp32" else "f64",
            "data": ("synthetic (toy_function on a seeded design)" if cand[0] == "grid" else
                     "synthetic (toy_function_3d on a seeded design drawn from the Sobol set)"),
            "config": {"workload": cfg["workload"], "n_train": n, "n_cand_per_gpu": per_rank,
                       "n_cand_total": total, "n_objectives": n_obj, "dim": d, "topq": q,
                       "parallelism": f"candidate-shard x{world}", "step_launch": step_launch,
                       "candidate_offset": offset},
            "selected": [int(i) for i in sel[1]],
        }
        if kernel_timed:
            # the fused kernel's own throughput and traffic (its event-timed launches)
            f = flops_per_candidate(n, n_obj, d)
            fx = executed_mfma_flops_per_candidate(args.mode, n, n_obj)
            executed = fx * per_rank / (k_ms * 1e-3) / 1e12
            ref_equiv = f * per_rank / (k_ms * 1e-3) / 1e12
            peak = PEAK_F32_MATRIX_TFLOPS if args.mode == "fp32" else PEAK_F64_MATRIX_TFLOPS
            # algorithmic HBM bytes per candidate: outputs written (+ explicit coordinates read)
            n_out = sum(1 if k == "acq" else n_obj for k in outputs)
            alg_bytes = (8 * n_out + (0 if cand[0] == "grid" else 8 * d)) * per_rank
            # the PMC summary key: the config in its default precision, "-<mode>" otherwise
            pmc_key = args.config if args.mode == ("fp32" if args.config == "C5" else "auto") \
                else f"{args.config}-{args.mode}"
            traffic, traffic_src = pmc_traffic(pmc_key) if args.acq == "sum_ucb" else \
                (None, "not measured: the committed PMC passes run the sum-of-UCB step (this step writes "
                       "the per-objective UCB the exact HVI reads)")
            if world > 1 and traffic is not None:
                # the committed PMC summaries are single-GPU runs over the whole candidate set: not
                # this rank's per-launch traffic
                traffic, traffic_src = None, (f"not measured per rank: {traffic_src} is a single-GPU "
                                              f"summary of the whole candidate set")
            res["roofline"] = {"bound": "mfma", "achieved": executed, "peak": peak, "unit": "TFLOP/s",
                               "frac": executed / peak,
                               "flops_basis": f"executed MFMA flops per candidate ({fx}; "
                                              f"{'upper form' if args.mode != 'dense' else 'dense form'})",
                               "traffic": traffic,
                               "traffic_source": traffic_src or "no PMC summary of this libbo_amd.so build",
                               "algorithmic_bytes": alg_bytes,
                               "traffic_ratio": (traffic / alg_bytes) if traffic else None,
                               "kernel": (f"cm32_predict_kernel<{2 if d <= 2 else 6}>" if args.mode == "fp32" else
                                          f"cm_predict_kernel<{2 if d <= 2 else 6}, {'true' if cand[0] == 'grid' else 'false'}, "
                                          f"{'true' if args.mode == 'auto' else 'false'}>"),
                               "kernel_ms": k_ms,
                               "formulation": ("upper: q = 2 k.(U k), U = triu((K^-1 + K^-T)/2), diag/2" if args.mode == "auto"
                                               else "upper form in f32 (mu, q accumulated in f32, the rest f64)"
                                               if args.mode == "fp32" else "dense: q = k^T (K^-1 k)"),
                               "executed_mfma_flops_per_candidate": fx,
                               "ref_flops_per_candidate": f,
                               "ref_flop_equiv_tflops": ref_equiv}
        if args.acq == "hvi":
            torch.cuda.synchronize()
            hms = float(np.mean([a.elapsed_time(b) for a, b in hvi_ev[-args.steps:]]))
            hb = (8 * n_obj + 8) * per_rank
            res["front_hypervolume"] = {"value": hv_front, "reference_point": ref_pt.tolist(),
                                        "method": f"bo_box_volume_sum over this rank's share of the "
                                                  f"{n_boxes[0]} boxes + all_reduce(SUM) over {world} rank(s)"}
            # device time per call as select_standalone takes it: the step's masked call replayed
            # as one HIP graph (no host launch gaps), after the timed region (--full)
            hvi_graph_ms = None
            if args.full and not args.hvi_unmasked:
                boxes_g = torch.as_tensor(hypervolume_boxes(front_y, ref_pt), device=dev)

                def hvi_call(strm):
                    bo._lib.check(lib.bo_hvi_select_topq_masked(
                        out["acq"].data_ptr(), out["ucb"].data_ptr(), per_rank, per_rank, n_obj, shift, scale,
                        boxes_g.data_ptr(), boxes_g.shape[0], offset, hvi_mask.ptr, q, rec.data_ptr(),
                        rec.data_ptr() + 8 * q, sel_ws.data_ptr(), sel_ws.numel(), strm), "hvi_select_masked")
                side = torch.cuda.Stream(dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                gh = torch.cuda.CUDAGraph()
                with torch.cuda.stream(side):
                    hvi_call(side.cuda_stream)
                    with torch.cuda.graph(gh, stream=side):
                        for _ in range(20):
                            hvi_call(side.cuda_stream)
                torch.cuda.current_stream(dev).wait_stream(side)
                gh.replay()
                torch.cuda.synchronize()
                g0, g1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                g0.record()
                gh.replay()
                g1.record()
                torch.cuda.synchronize()
                hvi_graph_ms = g0.elapsed_time(g1) / 20
            in_step_ms = hms
            if hvi_graph_ms is not None:
                hms = hvi_graph_ms
            res["hvi_select"] = {"kernels": (f"select_small_kernel<{n_obj}, 4> + select_rounds_merge_kernel" if q <= 4 else
                                             f"select_stream_kernel<{n_obj}, 4> + bo_topq_merge_kernel")
                                            + " (exact HVI + top-q, one pass)",
                                 "timing": ("HIP-graph replay of the masked call, device time per call (as select_standalone)"
                                            if hvi_graph_ms is not None else "event pair around the step's call"),
                                 "in_step_event_ms": in_step_ms,
                                 "exclusion": ("per-call hash set of the points (bo_hvi_select_topq)" if args.hvi_unmasked
                                               else "persistent exclusion mask (bo_hvi_select_topq_masked)"),
                                 "excl_mask": None if args.hvi_unmasked else mask_ms,
                                 "ms": hms, "n_boxes": n_boxes[0], "front_points": int(front_y.shape[0]),
                                 "bytes_per_candidate": 8 * n_obj + 8,
                                 "achieved_GBps": hb / (hms * 1e-3) / 1e9,
                                 "hbm_frac": hb / (hms * 1e-3) / 1e9 / 8000.0}
        if args.full and args.acq == "sum_ucb" and q <= 16:
            res["select_standalone"] = standalone_select(lib, bo, out["acq"], cands, offset, per_rank, xd,
                                                         q, dev, local_sel)
        if args.full and world == 1 and not args.no_cpu_baseline and args.acq == "sum_ucb":
            if cand[0] == "grid":
                side = cand[2]

                def points(lo, hi):
                    lin = np.arange(lo, hi)
                    return np.stack([lin // side, lin % side], axis=1).astype(np.float64)
                label = f"{args.config} grid"
            else:
                def points(lo, hi):
                    return cands.points(np.arange(lo, hi))
                label = f"{args.config} Sobol set"
            cb, cpu_acq, cpu_sel = cpu_baseline(x, y, pm, pv, ls, betas, kinv, points, label, q,
                                                max_cand=per_rank,
                                                full_limit=per_rank if args.cpu_full else 1 << 21)
            res["cpu_baseline"] = cb
            # parity of the timed run's own outputs against the CPU reference (outside the timing)
            done = cpu_acq.size
            gpu_acq = out["acq"][:done].cpu().numpy()
            res["acq_max_err_vs_cpu"] = float(np.max(np.abs(gpu_acq - cpu_acq) / np.maximum(1.0, np.abs(cpu_acq))))
            if done == per_rank:
                excluded = _rows_in(points(0, done), x) if cand[0] != "grid" else _grid_excluded(x, side, done)
                res["selection_matches_cpu"] = selection_check(sel[1], cpu_acq, excluded, q)
                res["cpu_selected"] = [int(i) for i in cpu_sel]
            else:
                res["selection_matches_cpu"] = None   # sample shorter than the shard
        if use_dist:
            res["collectives"] = {"backend": dist.get_backend(), "world_size": dist.get_world_size(),
                                  "exchange": "all_gather_into_tensor of the 16-B top-q records per step"}
        print(json.dumps(res), flush=True)
    if use_dist:
        dist.destroy_process_group()


def standalone_select(lib, bo, acq, cands, offset, n, xd, q, dev, fused_sel, reps=20):
    """bo_select_topq (select_next_batch over a stored acquisition array, acquisition.py:116-144)
    on this shard's acq array from the timed run, with the evaluated points excluded: device time
    per call (one-pass selection kernel + the final merge, HIP-graph replayed), its HBM rate on the
    8 B per candidate it must read, and whether it selects what the fused kernel selected.  `ms`
    is the masked call (bo_select_topq_masked over the shard's persistent exclusion mask, which
    the loop builds once and extends by q points per iteration -- both timed, `excl_mask`);
    `per_call_exclusion` the same selection with the points' hash set built inside the call
    (bo_select_topq).  Outside the timed region."""
    import ctypes
    import torch
    from bayesopt_smart_amd.acquisition import ExclusionMask
    ws = torch.empty(lib.bo_select_topq_workspace_size(n, q), dtype=torch.uint8, device=dev)
    tv = torch.empty(q, dtype=torch.float64, device=dev)
    ti = torch.empty(q, dtype=torch.int64, device=dev)
    glo = (ctypes.c_int64 * 8)(*((list(cands.lo) if cands.lo else []) + [0] * (8 - len(cands.lo or []))))
    gsh = (ctypes.c_int64 * 8)(*((list(cands.shape) if cands.shape else []) + [1] * (8 - len(cands.shape or []))))
    carg = cands.tensor[offset:].data_ptr() if cands.kind in ("i64", "f64") else cands.cand_arg
    xh = xd.cpu().numpy()
    mask = ExclusionMask(cands, offset, n, dev)
    mask_ms = {}
    for tag, rows in (("build_ms", xh[:-q]), ("extend_q_ms", xh)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        mask.update(rows)
        e1.record()
        torch.cuda.synchronize()
        mask_ms[tag] = e0.elapsed_time(e1)

    def call_points(strm):
        bo._lib.check(lib.bo_select_topq(acq.data_ptr(), n, cands.kind_code, carg, glo, gsh, cands.dim,
                                         offset, xd.data_ptr(), xd.shape[0], q, tv.data_ptr(),
                                         ti.data_ptr(), ws.data_ptr(), ws.numel(), strm), "select")

    def call_masked(strm):
        bo._lib.check(lib.bo_select_topq_masked(acq.data_ptr(), n, offset, mask.ptr, q, tv.data_ptr(),
                                                ti.data_ptr(), ws.data_ptr(), ws.numel(), strm), "select_masked")

    def timed(call):
        call(bo.device.stream_handle(dev))
        torch.cuda.synchronize()
        got = ti.cpu().numpy()
        # the reps calls replayed as one HIP graph: device time per call, no host launch cost
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            call(side.cuda_stream)
            with torch.cuda.graph(g, stream=side):
                for _ in range(reps):
                    call(side.cuda_stream)
        torch.cuda.current_stream(dev).wait_stream(side)
        g.replay()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps, bool(np.array_equal(got[got >= 0], np.asarray(fused_sel)))

    ms_p, ok_p = timed(call_points)
    ms, ok = timed(call_masked)
    return {"kernels": ("select_small_kernel<0, 4> + select_rounds_merge_kernel" if q <= 4 else
                        "select_stream_kernel<0, 8> + bo_topq_merge_kernel") + " (HIP-graph replay)",
            "exclusion": "persistent exclusion mask (bo_select_topq_masked)",
            "ms": ms, "bytes": 8 * n, "achieved_GBps": 8 * n / (ms * 1e-3) / 1e9,
            "hbm_frac": 8 * n / (ms * 1e-3) / 1e9 / 8000.0,
            "excl_mask": mask_ms,
            "per_call_exclusion": {"ms": ms_p, "matches_fused_selection": ok_p},
            "matches_fused_selection": ok and ok_p}


def _rows_in(pts, x):
    """Mask of the rows of pts equal (all coordinates) to some row of x."""
    v = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.dtype((np.void, 8 * a.shape[1]))).ravel()  # noqa: E731
    return np.isin(v(pts), v(x))


def _grid_excluded(x, side, m):
    """Evaluated grid points as a mask over the 'ij' grid's linear index."""
    ex = np.zeros(m, dtype=bool)
    lin = x[:, 0].astype(np.int64) * side + x[:, 1].astype(np.int64)
    ex[lin[(lin >= 0) & (lin < m)]] = True
    return ex


if __name__ == "__main__":
    main()

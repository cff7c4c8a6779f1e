"""bench.py's command line: a plain run does the timed steps only (the fields of --full are
absent), --steps sets the number of timed steps, --dump-outputs writes what the last timed step
computed -- identical from run to run -- within its size limit, as float64 .npy files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FULL_ONLY = ("roofline", "select_standalone", "cpu_baseline", "acq_max_err_vs_cpu", "selection_matches_cpu")


@pytest.mark.parametrize("n_cand, per_cand", [(1 << 20, 5), (1 << 21, 7), (1 << 22, 7), (1000, 7)])
def test_dump_sample_is_fixed_and_within_the_limit(n_cand, per_cand):
    import bench
    idx = bench.dump_sample_index(n_cand, per_cand)
    if 8 * per_cand * n_cand + (1 << 16) <= bench.DUMP_LIMIT_BYTES:
        assert idx is None                                   # everything fits: no sampling
        return
    assert idx.dtype == np.int64 and np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < n_cand
    assert 8 * (per_cand + 1) * idx.size + (1 << 16) <= bench.DUMP_LIMIT_BYTES
    assert 8 * (per_cand + 1) * (idx.size + 1) + (1 << 16) > bench.DUMP_LIMIT_BYTES   # as many as fit
    np.testing.assert_array_equal(idx, bench.dump_sample_index(n_cand, per_cand))


def test_dump_limit_is_64_mb():
    import bench
    assert bench.DUMP_LIMIT_BYTES <= 64 * 1000 * 1000


def _bench(*args):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", *args], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_dumps_its_last_step(tmp_path):
    """C2 (262,144 candidates: the quickest config) twice: the plain line, the dumped arrays
    against the line and against each other."""
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    res = _bench("--config", "C2", "--steps", "3", "--warmup", "1", "--dump-outputs", a)
    _bench("--config", "C2", "--steps", "2", "--warmup", "1", "--dump-outputs", b)
    assert res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(res["config"]["n_cand_total"] / (res["ms_per_step"] * 1e-3))
    assert res["unit"] == "candidate-points/sec" and res["higher_is_better"] is True and res["dtype"] == "f64"
    assert not [k for k in FULL_ONLY if k in res]
    m, n_obj = res["config"]["n_cand_per_gpu"], res["config"]["n_objectives"]
    shapes = {"mu": (n_obj, m), "var": (n_obj, m), "ucb": (n_obj, m), "acq": (m,),
              "selected_values": (3,), "selected_indices": (3,)}
    assert sorted(os.listdir(a)) == sorted(f"{k}.npy" for k in shapes)
    assert sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a)) <= 64 * 1000 * 1000
    for name, shape in shapes.items():
        x = np.load(os.path.join(a, f"{name}.npy"))
        assert x.dtype == np.float64 and x.shape == shape, name
        assert np.all(np.isfinite(x)), name
        np.testing.assert_array_equal(x, np.load(os.path.join(b, f"{name}.npy")), err_msg=name)
    sel = np.load(os.path.join(a, "selected_indices.npy")).astype(np.int64)
    assert sel.tolist() == res["selected"]
    np.testing.assert_array_equal(np.load(os.path.join(a, "acq.npy"))[sel],
                                  np.load(os.path.join(a, "selected_values.npy")))

"""Child of tests/test_gpu_ts.py, launched by torch.distributed.run with one rank: the loop with
batch_strategy="ts" for both acquisitions, first with the RCCL process group and
BO_FORCE_COLLECTIVES=1 (every draw's record block goes through exchange_topq_rec's all_gather), then
again after destroy_process_group; prints both trajectories."""
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, sys.argv[1])
os.environ["BO_FORCE_COLLECTIVES"] = "1"
dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
torch.cuda.set_device(dev)
dist.init_process_group("nccl", device_id=dev)

from bayesopt_smart_amd.bayesian_optimization import BayesianOptimization  # noqa: E402
from bayesopt_smart_amd.distributed import collectives_on  # noqa: E402


def toy(x):
    return np.array([-((x[0] - 12) ** 2) / 50.0 + 3.0, -((x[1] - 118) ** 2) / 40.0 + 2.0 + 0.02 * x[0]])


def run():
    out = {}
    for kind in ("sum_ucb", "hvi"):
        np.random.seed(42)
        opt = BayesianOptimization(toy, [(-5, 28), (100, 131)], n_objectives=2, initial_samples=8, n_iterations=2,
                                   batch_size=4, betas=np.array([2.0, 2.0]), acquisition=kind, device=dev,
                                   batch_strategy="ts", ts_features=128, ts_seed=7,
                                   reference_point=[-30.0, -30.0])
        opt.optimize()
        out[kind] = opt.x_vector.tolist()
    return out


res = {"backend": dist.get_backend(), "collectives": collectives_on()}
res["rccl"] = run()
dist.destroy_process_group()
res["collectives_after"] = collectives_on()
res["plain"] = run()
print("RESULT " + json.dumps(res))

"""Child of tests/test_gpu_logehvi.py, launched by torch.distributed.run with one rank per device: the loop
with acquisition="logehvi" over the RCCL process group (one rank: BO_FORCE_COLLECTIVES=1 from the parent, so
the records' all_gather runs); every rank prints its trajectory."""
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, sys.argv[1])
dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
torch.cuda.set_device(dev)
dist.init_process_group("nccl", device_id=dev)

from bayesopt_smart_amd.bayesian_optimization import BayesianOptimization  # noqa: E402
from bayesopt_smart_amd.distributed import collectives_on  # noqa: E402


def toy2(x):
    a, b = (x[0] + 5.0) / 33.0, (x[1] - 100.0) / 31.0
    return np.array([-(a - 0.3) ** 2 - (b - 0.6) ** 2, np.sin(3.0 * a) + 0.5 * b])


np.random.seed(42)
opt = BayesianOptimization(toy2, [(-5, 28), (100, 131)], n_objectives=2, initial_samples=8, n_iterations=3,
                           batch_size=3, acquisition="logehvi", reference_point=[-3.0, -3.0], device=dev)
opt.optimize()
res = {"rank": dist.get_rank(), "collectives": collectives_on(), "x": opt.x_vector.tolist()}
dist.destroy_process_group()
print("RESULT " + json.dumps(res), flush=True)

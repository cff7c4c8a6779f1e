"""sha256 of the outputs of every consumer of the candidate decode (csrc/bo_cand.h), with the library
named by BO_AMD_LIB: two builds that must compute the same bits (a refactor of the decode) are
checked by comparing the printed digests.  The shards and the runners are those of
tests/test_gpu_cand_decode.py (tests/cand_cases.py): every form of every shard, through the top-q
selection with the per-call exclusion, ExclusionMask.excluded(), select_batch_bucb and
select_batch_kb (return_details=True) and sample_paths; and select_indices over a whole grid.

    BO_AMD_LIB=.../lib.so python scripts/cand_outputs_sha.py"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import bayesopt_smart_amd as bo  # noqa: E402
import cand_cases as C  # noqa: E402


def digest(out):
    h = hashlib.sha256()
    for k in sorted(out):
        h.update(k.encode() + np.ascontiguousarray(out[k]).tobytes())
    return h.hexdigest()[:24]


lib = os.path.basename(os.environ.get("BO_AMD_LIB", "libbo_amd.so"))
for name in C.CASES:
    c = C.case(name)
    for label, cands, offset in C.forms(c):
        for consumer, run in C.RUNNERS.items():
            kws = [{"q": C.Q}, {"q": 16}] if consumer == "topq" else [{}]
            for kw in kws:
                print(f"{lib} {name} {label} {consumer}{kw.get('q', '')}: {digest(run(c, cands, offset, **kw))}", flush=True)
# select_indices walks the whole set: the 70 x 90 grid, the shard's acquisition values repeated over it
c = C.case("grid32")
acq = torch.as_tensor(np.resize(c["acq"], c["implicit"].n), device="cuda")
idx = bo.acquisition.select_indices(acq, c["implicit"], c["ev"], 64)    # two rounds of the per-call exclusion
print(f"{lib} grid32 grid select_indices64: {digest({'idx': idx})}", flush=True)

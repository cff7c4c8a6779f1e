"""The candidate decode (csrc/bo_cand.h) gives the same point whatever form the point is given in:
every consumer -- the top-q selection with the per-call exclusion, the exclusion mask's update, the
hallucinated-observation batches and the posterior draws -- is run over one shard as a grid (or the
Sobol sequence) and as explicit int64 / f64 rows, and the outputs must agree bit for bit
(tests/cand_cases.py holds the shards and the runners).  The other tests compare each consumer
with a host reference within a tolerance, on grids whose axes are below 2^31; here the 64-bit
decode meets an axis above 2^31, a shard across a row boundary and a padded coordinate."""
import numpy as np
import pytest

import cand_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def device():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def assert_forms_agree(name, consumer, **kw):
    c = C.case(name)
    outs = [(label, C.RUNNERS[consumer](c, cands, offset, **kw)) for label, cands, offset in C.forms(c)]
    label0, first = outs[0]
    for label, out in outs[1:]:
        for key, want in first.items():
            assert out[key].dtype == want.dtype and out[key].shape == want.shape, (name, key, label)
            assert out[key].tobytes() == want.tobytes(), f"{name}: {key} of {label} differs from {label0}"
    return c, first


@pytest.mark.parametrize("q", [C.Q, 16])                     # the small-q kernel and the streaming one
@pytest.mark.parametrize("name", C.CASES)
def test_topq_with_per_call_exclusion(name, q):
    c, got = assert_forms_agree(name, "topq", q=q)
    excl = np.zeros(C.COUNT, dtype=bool)
    excl[c["hot"]] = True                                     # the best 40 are evaluated points
    excl |= (c["pts"][:, None, :] == c["x"][None, :, :]).all(-1).any(1)
    order = np.lexsort((np.arange(C.COUNT), -np.where(excl, -np.inf, c["acq"])))
    np.testing.assert_array_equal(got["top_idx"], order[:q])


@pytest.mark.parametrize("name", C.CASES)
def test_mask_update(name):
    c, got = assert_forms_agree(name, "mask")
    want = (c["pts"][:, None, :] == c["ev"][None, :, :]).all(-1).any(1)
    assert want.sum() >= 40
    np.testing.assert_array_equal(got["excluded"], want)


@pytest.mark.parametrize("name", C.CASES)
def test_bucb(name):
    c, got = assert_forms_agree(name, "bucb")
    assert len(set(got["top_idx"])) == C.Q and got["top_idx"].min() >= 0
    assert (got["var"] < c["var"]).any() and np.isfinite(got["var"]).all()   # the update ran


@pytest.mark.parametrize("name", C.CASES)
def test_sample_paths(name):
    _, got = assert_forms_agree(name, "paths")
    assert np.isfinite(got["paths"]).all() and np.ptp(got["paths"]) > 0.0

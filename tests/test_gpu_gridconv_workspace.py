"""GPU tests of the grid-convolution path's workspace layout (conv_layout, bo_predict_impl.h): a call
run in a workspace of exactly bo_predict_workspace_size bytes between two guard pages writes neither
page, and every output is bit for bit that of the same call on the package's ordinary workspace.

The buffer is filled with 0xA5 (tickets and counters far past the items, offsets out of range), the
workspace starts at its byte 4096 (256-aligned) and ws_bytes is the exact size."""

import numpy as np
import pytest

import gridconv_model as G
import test_gpu_gridconv_sched as SCH

pytestmark = pytest.mark.gpu

ALL = SCH.ALL
GUARD = 4096
FILL = 0xA5
WIDE_SHAPE = (17, 65)   # C = 65: Cpad = 128, LT = 144, 2C - 1 = 129 one past a multiple of 16


@pytest.fixture(scope="module")
def bo():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import bayesopt_smart_amd as bo
    bo._lib.load()
    return bo


def _wide():
    # 37 points, 8 objectives (BO_MAX_OBJ: every ticket line in use); run with q = 48 (BO_MAX_TOPQ)
    rng = np.random.default_rng(51)
    lin = rng.choice(WIDE_SHAPE[0] * WIDE_SHAPE[1], size=37, replace=False)
    return WIDE_SHAPE, SCH._make(np.stack([lin // WIDE_SHAPE[1], lin % WIDE_SHAPE[1]], axis=1), 8, 51)


_PROBLEMS = {}


def _problem(name):
    if name not in _PROBLEMS:
        _PROBLEMS[name] = _wide() if name == "wide" else SCH._BUILDERS[name]()
    return _PROBLEMS[name]


class _Guarded:
    """A prepared call whose workspace is the middle of a guarded buffer of its own."""

    def __init__(self, bo, d, cands, q, mode, offset=0, count=None):
        import torch
        self.call = bo.predict.predict_acquire(d["x"], d["y"], d["Kinv"], cands, d["pm"], d["pv"], d["ls"], d["betas"],
                                               outputs=ALL, topq=q, offset=offset, count=count, mode=mode, prepare=True)
        self.nbytes = int(bo._lib.load().bo_predict_workspace_size(self.call._desc))
        assert self.nbytes > 0 and self.nbytes % 256 == 0
        self.buf = torch.empty(self.nbytes + 2 * GUARD, dtype=torch.uint8, device=self.call._ws.device)
        assert (self.buf.data_ptr() + GUARD) % 256 == 0
        self.call._ws = self.buf
        self.call._ws_ptr, self.call._ws_n = self.buf.data_ptr() + GUARD, self.nbytes
        self.fill()

    def fill(self):
        import torch
        for t in self.call.res.values():
            if isinstance(t, torch.Tensor):
                t.zero_()
        self.buf.fill_(FILL)

    def outputs(self):
        """Synchronise, check the guards, return the outputs."""
        import torch
        torch.cuda.synchronize()
        assert bool((self.buf[:GUARD] == FILL).all()), "written below the workspace"
        assert bool((self.buf[GUARD + self.nbytes:] == FILL).all()), "written past the workspace"
        return {k: v.cpu().numpy() for k, v in self.call.res.items() if not k.startswith("_")}


def _bit_equal(a, b):
    assert set(a) == set(b) == set(ALL) | {"top_idx", "top_val"}
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def _check(bo, name, q, offset=0, count=None):
    shape, d = _problem(name)
    assert G.conv_planned(shape, d["x"].shape[0], len(d["pm"]), offset, count, mode="auto-conv")
    cands = SCH._cands(bo, shape)
    g = _Guarded(bo, d, cands, q, "auto-conv", offset, count)
    g.call()
    _bit_equal(g.outputs(), SCH._call(bo, d, cands, q, offset=offset, count=count))
    return shape, d


def test_edge_problem(bo):
    _check(bo, "edges", 3)


def test_one_point(bo):
    _check(bo, "single", 3)


def test_every_ticket_line_and_the_largest_lists(bo):
    shape, d = _check(bo, "wide", 48)
    C = shape[1]
    assert len(d["pm"]) == bo._lib.MAX_OBJ and bo._lib.MAX_TOPQ == 48
    assert -(-C // 64) * 64 == 128 and -(-(2 * C - 1) // 16) * 16 == 144 and (2 * C - 1) % 16 == 1


def test_shard_inside_grid_rows(bo):
    C = WIDE_SHAPE[1]
    offset, count = 3 * C + 7, 9 * C + 11
    assert offset % C != 0 and (offset + count) % C != 0
    _check(bo, "wide", 48, offset, count)


@pytest.mark.parametrize("name,tickets", [("clusters-static", False), ("clusters-tickets", True)])
def test_with_and_without_tickets(bo, name, tickets):
    shape, d = _problem(name)
    items, wgs, dyn = SCH._acc_schedule(shape, len(d["pv"]), SCH._cus())
    assert dyn == tickets and (items > 4 * wgs) == tickets
    _check(bo, name, 16)


def test_off_grid_point_runs_the_chunk_major_kernel_in_the_same_workspace(bo):
    """Planned, turned down by the device flag: the chunk-major kernel's outputs, bit for bit."""
    shape, d = _problem("edges")
    d = dict(d, x=d["x"].copy())
    d["x"][4, 0] += 0.5
    assert G.conv_planned(shape, d["x"].shape[0], len(d["pm"]), mode="auto-conv")
    cands = SCH._cands(bo, shape)
    g = _Guarded(bo, d, cands, 3, "auto-conv")
    g.call()
    _bit_equal(g.outputs(), SCH._call(bo, d, cands, 3, mode="auto-noconv"))


def test_graph_replays(bo):
    """Two replays of one captured graph, the whole buffer refilled before each."""
    shape, d = _problem("edges")
    cands = SCH._cands(bo, shape)
    g = _Guarded(bo, d, cands, 3, "auto-conv")
    replay = g.call.graphed()
    runs = []
    for _ in range(2):
        g.fill()
        replay()
        runs.append(g.outputs())
    _bit_equal(runs[0], runs[1])
    _bit_equal(runs[0], SCH._call(bo, d, cands, 3))
